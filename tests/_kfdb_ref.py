"""Plain-Python restatement of what place recognition rests on, the checker of tests/test_gpu_bowvec.py and tests/test_gpu_table_bow.py.
It imports nothing from the package.

  * DBoW2 BowVector::addWeight / normalize(L1) and L1Scoring::score on Python floats (IEEE double), strictly sequential loops - no
    numpy.sum, whose pairwise order is different.  DBoW2 is an empty submodule in the reference; these follow upstream DBoW2 (parity
    unpinned, like the BoW descent).
  * KeyFrameDatabase::add / erase / DetectLoopCandidates / DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:40-309) and the
    minScore loop of LoopClosing::DetectLoop (src/LoopClosing.cc:142-155) line by line on dicts and lists, with a real per-word inverted
    file and numpy.float32 wherever the reference says `float`.

KeyFrame::mRelocScore / mLoopScore are members that outlive a query; the reference never initialises them (KeyFrame.cc:40), here they
start at 0.

flip= (bow_vector, l1_score and the two detect_* methods) selects ONE wrong variant of ONE rule; a constructed scene of tests/_kfdb_scenes.py
is only worth its name when the matching flip moves its answer (tests/test_kfdb_ref_cpu.py).  FLIPS lists them."""
import numpy as np

F32 = np.float32


# ---------------- DBoW2 ----------------
BOW_FLIPS = ("count_times_weight", "norm_reversed")
SCORE_FLIPS = ("sum_reversed", "sum_pairwise")
DETECT_FLIPS = ("common_ge", "common_round", "min_score_gt", "retain_ge", "takeover_ge", "acc_double", "acc_reversed", "reloc_fresh_scores",
                "loop_counts_ungated", "order_by_slot")
FLIPS = BOW_FLIPS + SCORE_FLIPS + DETECT_FLIPS


def _known(flip, allowed):
    if flip is not None and flip not in allowed:
        raise ValueError("unknown flip %r" % (flip,))


def bow_vector(leaf, weight, word_id, flip=None):
    """TemplatedVocabulary::transform's BowVector: for every feature, in order, if(w > 0) v.addWeight(word, w); then v.normalize(L1).
    Returns {word: value} in ascending word order"""
    _known(flip, BOW_FLIPS)
    bow, count = {}, {}
    for lf in leaf:
        w = float(weight[lf])
        if w > 0:
            wid = int(word_id[lf])
            if wid in bow:
                bow[wid] = bow[wid] + w   # BowVector::addWeight: vit->second += v
            else:
                bow[wid] = w              # ... or insert(value_type(id, v))
            count[wid] = count.get(wid, 0) + 1
            if flip == "count_times_weight":
                bow[wid] = count[wid] * w
    bow = dict(sorted(bow.items()))       # std::map order
    norm = 0.0
    for v in (reversed(list(bow.values())) if flip == "norm_reversed" else bow.values()):   # BowVector::normalize: norm += fabs(it->second), map order
        norm = norm + abs(v)
    if norm > 0.0:
        for k in bow:
            bow[k] = bow[k] / norm
    return bow


def _tree_sum(t):
    if len(t) == 1:
        return t[0]
    return _tree_sum(t[:len(t) // 2]) + _tree_sum(t[len(t) // 2:])


def l1_score(v1, v2, flip=None):
    """L1Scoring::score(v1, v2) over two ascending {word: value} maps: (words in common, score, smallest shared word or -1).
    The score of vectors that share nothing is 0.0"""
    _known(flip, SCORE_FLIPS)
    k1, k2 = list(v1.keys()), list(v2.keys())
    i = j = 0
    terms = []
    first = -1
    while i < len(k1) and j < len(k2):
        if k1[i] == k2[j]:
            vi, wi = v1[k1[i]], v2[k2[j]]
            terms.append(abs(vi - wi) - abs(vi) - abs(wi))   # score += fabs(vi - wi) - fabs(vi) - fabs(wi)
            if first < 0:
                first = k1[i]
            i += 1
            j += 1
        elif k1[i] < k2[j]:
            i += 1                                       # (upstream: lower_bound; the visited pairs are the same)
        else:
            j += 1
    s = 0.0
    if flip == "sum_pairwise" and terms:
        s = s + _tree_sum(terms)
    else:
        for t in (reversed(terms) if flip == "sum_reversed" else terms):
            s = s + t
    common = len(terms)
    return common, (-s / 2.0 if common else 0.0), first


def score(v1, v2):
    return l1_score(v1, v2)[1]


# ---------------- KeyFrameDatabase.cc ----------------
class KF:
    def __init__(self, kid, bow):
        self.id, self.bow = kid, bow
        self.loop_query, self.loop_words, self.loop_score = None, 0, F32(0)
        self.reloc_query, self.reloc_words, self.reloc_score = None, 0, F32(0)
        self.reloc_scored = None          # the query that last wrote reloc_score (what the flip reloc_fresh_scores looks at)


COUNTERS = ("common_eq", "min_score_eq", "retain_eq", "takeover_eq", "stale_used", "below_gate_neighbour")


def _min_common(max_common, flip):
    x = F32(max_common) * F32(0.8)
    return int(np.floor(x + F32(0.5))) if flip == "common_round" else int(x)   # int minCommonWords = maxCommonWords*0.8f


def _passes_common(words, min_common, flip, trace):
    if trace is not None and words == min_common:
        trace["common_eq"] += 1
    return words >= min_common if flip == "common_ge" else words > min_common


class _Acc:
    """float accScore = si; accScore += score of a neighbour.  Flip acc_double: kept in double, rounded to float once at the end"""

    def __init__(self, si, flip):
        self.double = flip == "acc_double"
        self.v = float(si) if self.double else si

    def add(self, x):
        self.v = self.v + float(x) if self.double else F32(self.v + x)

    def value(self):
        return F32(self.v)


def _takes_over(s2, best_score, flip, trace):
    if trace is not None and s2 == best_score:
        trace["takeover_eq"] += 1
    return s2 >= best_score if flip == "takeover_ge" else s2 > best_score


class KeyFrameDatabaseRef:
    def __init__(self):
        self.inverted = {}   # word -> list of KF, insertion order
        self.kfs = {}
        self._query = 0

    def add(self, kid, bow):                       # :40-46
        kf = self.kfs.get(kid) or KF(kid, bow)
        kf.bow = bow
        self.kfs[kid] = kf
        for w in bow:
            self.inverted.setdefault(w, []).append(kf)

    def erase(self, kid):                          # :48-67
        kf = self.kfs[kid]
        for w in kf.bow:
            lst = self.inverted.get(w, [])
            for n, o in enumerate(lst):
                if o is kf:
                    del lst[n]
                    break

    @staticmethod
    def _start(trace, sharing):
        if trace is not None:
            trace.update(sharing=[k.id for k in sharing], scored=[], passed=[], acc=[])
            trace.update({c: 0 for c in COUNTERS})

    def detect_loop_candidates(self, bow, minScore, connected, best_covisibles, trace=None, flip=None):   # :76-197
        """bow: the query keyframe's BowVector; connected: ids; best_covisibles(id) -> ids.  trace (a dict) receives the intermediate lists
        and the counters of equalities met (COUNTERS)"""
        _known(flip, DETECT_FLIPS)
        minScore = F32(minScore)
        self._query += 1
        qid = ("loop", self._query)
        connected = set(connected)
        sharing = []
        for w in bow:
            for kfi in self.inverted.get(w, []):
                if kfi.loop_query != qid:
                    kfi.loop_words = 0
                    if kfi.id not in connected:
                        kfi.loop_query = qid
                        sharing.append(kfi)
                kfi.loop_words += 1
        if flip == "order_by_slot":
            sharing.sort(key=lambda k: k.id)
        self._start(trace, sharing)
        if not sharing:
            return []
        max_common = 0
        for kfi in sharing:
            if kfi.loop_words > max_common:
                max_common = kfi.loop_words
        min_common = _min_common(max_common, flip)
        score_and_match = []
        for kfi in sharing:
            if _passes_common(kfi.loop_words, min_common, flip, trace):
                si = F32(score(bow, kfi.bow))
                kfi.loop_score = si
                if trace is not None:
                    trace["scored"].append(kfi.id)
                    trace["min_score_eq"] += int(si == minScore)
                if (si > minScore) if flip == "min_score_gt" else (si >= minScore):
                    score_and_match.append((si, kfi))
        if trace is not None:
            trace["passed"] = [k.id for _, k in score_and_match]
            trace["min_common"] = min_common
        if not score_and_match:
            return []
        acc_and_match = []
        best_acc = minScore
        for si, kfi in score_and_match:
            best_score, acc, best_kf = si, _Acc(si, flip), kfi
            covis = list(best_covisibles(kfi.id))
            for k2id in (reversed(covis) if flip == "acc_reversed" else covis):
                kf2 = self.kfs.get(k2id)
                if kf2 is None:
                    continue
                gated = kf2.loop_words > min_common
                if trace is not None and kf2.loop_query == qid and not gated:
                    trace["below_gate_neighbour"] += 1
                if kf2.loop_query == qid and (gated or flip == "loop_counts_ungated"):
                    acc.add(kf2.loop_score)
                    if _takes_over(kf2.loop_score, best_score, flip, trace):
                        best_kf, best_score = kf2, kf2.loop_score
            acc_and_match.append((acc.value(), best_kf))
            if acc.value() > best_acc:
                best_acc = acc.value()
        return self._retain(acc_and_match, best_acc, trace, flip)

    def detect_relocalization_candidates(self, bow, best_covisibles, trace=None, flip=None):   # :199-309
        _known(flip, DETECT_FLIPS)
        self._query += 1
        qid = ("reloc", self._query)
        sharing = []
        for w in bow:
            for kfi in self.inverted.get(w, []):
                if kfi.reloc_query != qid:
                    kfi.reloc_words = 0
                    kfi.reloc_query = qid
                    sharing.append(kfi)
                kfi.reloc_words += 1
        if flip == "order_by_slot":
            sharing.sort(key=lambda k: k.id)
        self._start(trace, sharing)
        if not sharing:
            return []
        max_common = 0
        for kfi in sharing:
            if kfi.reloc_words > max_common:
                max_common = kfi.reloc_words
        min_common = _min_common(max_common, flip)
        score_and_match = []
        for kfi in sharing:
            if _passes_common(kfi.reloc_words, min_common, flip, trace):
                si = F32(score(bow, kfi.bow))
                kfi.reloc_score = si
                kfi.reloc_scored = qid
                score_and_match.append((si, kfi))
        if trace is not None:
            trace["scored"] = trace["passed"] = [k.id for _, k in score_and_match]
            trace["min_common"] = min_common
        if not score_and_match:
            return []
        acc_and_match = []
        best_acc = F32(0)
        for si, kfi in score_and_match:
            best_score, acc, best_kf = si, _Acc(si, flip), kfi
            covis = list(best_covisibles(kfi.id))
            for k2id in (reversed(covis) if flip == "acc_reversed" else covis):
                kf2 = self.kfs.get(k2id)
                if kf2 is None or kf2.reloc_query != qid:
                    continue
                s2 = kf2.reloc_score              # :273-276: whatever the member holds, scored in this query or not
                if kf2.reloc_scored != qid:
                    if trace is not None:
                        trace["stale_used"] += 1
                    if flip == "reloc_fresh_scores":
                        s2 = F32(0)
                acc.add(s2)
                if _takes_over(s2, best_score, flip, trace):
                    best_kf, best_score = kf2, s2
            acc_and_match.append((acc.value(), best_kf))
            if acc.value() > best_acc:
                best_acc = acc.value()
        return self._retain(acc_and_match, best_acc, trace, flip)

    @staticmethod
    def _retain(acc_and_match, best_acc, trace, flip=None):
        min_retain = F32(0.75) * best_acc
        if trace is not None:
            trace["acc"] = [(float(a), k.id) for a, k in acc_and_match]
            trace["min_retain"] = float(min_retain)
            trace["retain_eq"] = sum(int(a == min_retain) for a, _ in acc_and_match)
        out, seen = [], set()
        for acc, kf in acc_and_match:
            if (acc >= min_retain) if flip == "retain_ge" else (acc > min_retain):
                if kf.id not in seen:
                    out.append(kf.id)
                    seen.add(kf.id)
        return out


def min_score_to_connected(bow, connected_bows):   # LoopClosing.cc:142-155
    min_score = F32(1)
    for b in connected_bows:
        sc = F32(score(bow, b))
        if sc < min_score:
            min_score = sc
    return min_score
