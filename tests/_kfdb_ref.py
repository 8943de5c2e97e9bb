"""Plain-Python restatement of what place recognition rests on, the checker of tests/test_gpu_bowvec.py and tests/test_gpu_table_bow.py.
It imports nothing from the package.

  * DBoW2 BowVector::addWeight / normalize(L1) and L1Scoring::score on Python floats (IEEE double), strictly sequential loops - no
    numpy.sum, whose pairwise order is different.  DBoW2 is an empty submodule in the reference; these follow upstream DBoW2 (parity
    unpinned, like the BoW descent).
  * KeyFrameDatabase::add / erase / DetectLoopCandidates / DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:40-309) and the
    minScore loop of LoopClosing::DetectLoop (src/LoopClosing.cc:142-155) line by line on dicts and lists, with a real per-word inverted
    file and numpy.float32 wherever the reference says `float`.

KeyFrame::mRelocScore / mLoopScore are members that outlive a query; the reference never initialises them (KeyFrame.cc:40), here they
start at 0."""
import numpy as np

F32 = np.float32


# ---------------- DBoW2 ----------------
def bow_vector(leaf, weight, word_id):
    """TemplatedVocabulary::transform's BowVector: for every feature, in order, if(w > 0) v.addWeight(word, w); then v.normalize(L1).
    Returns {word: value} in ascending word order"""
    bow = {}
    for lf in leaf:
        w = float(weight[lf])
        if w > 0:
            wid = int(word_id[lf])
            if wid in bow:
                bow[wid] = bow[wid] + w   # BowVector::addWeight: vit->second += v
            else:
                bow[wid] = w              # ... or insert(value_type(id, v))
    bow = dict(sorted(bow.items()))       # std::map order
    norm = 0.0
    for v in bow.values():                # BowVector::normalize: norm += fabs(it->second), map order
        norm = norm + abs(v)
    if norm > 0.0:
        for k in bow:
            bow[k] = bow[k] / norm
    return bow


def l1_score(v1, v2):
    """L1Scoring::score(v1, v2) over two ascending {word: value} maps: (words in common, score, smallest shared word or -1).
    The score of vectors that share nothing is 0.0"""
    k1, k2 = list(v1.keys()), list(v2.keys())
    i = j = 0
    s = 0.0
    common, first = 0, -1
    while i < len(k1) and j < len(k2):
        if k1[i] == k2[j]:
            vi, wi = v1[k1[i]], v2[k2[j]]
            s = s + (abs(vi - wi) - abs(vi) - abs(wi))   # score += fabs(vi - wi) - fabs(vi) - fabs(wi)
            if first < 0:
                first = k1[i]
            common += 1
            i += 1
            j += 1
        elif k1[i] < k2[j]:
            i += 1                                       # (upstream: lower_bound; the visited pairs are the same)
        else:
            j += 1
    return common, (-s / 2.0 if common else 0.0), first


def score(v1, v2):
    return l1_score(v1, v2)[1]


# ---------------- KeyFrameDatabase.cc ----------------
class KF:
    def __init__(self, kid, bow):
        self.id, self.bow = kid, bow
        self.loop_query, self.loop_words, self.loop_score = None, 0, F32(0)
        self.reloc_query, self.reloc_words, self.reloc_score = None, 0, F32(0)


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

    def detect_loop_candidates(self, bow, minScore, connected, best_covisibles, trace=None):   # :76-197
        """bow: the query keyframe's BowVector; connected: ids; best_covisibles(id) -> ids.  trace (a dict) receives the intermediate lists"""
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
        if trace is not None:
            trace.update(sharing=[k.id for k in sharing], scored=[], passed=[], acc=[])
        if not sharing:
            return []
        max_common = 0
        for kfi in sharing:
            if kfi.loop_words > max_common:
                max_common = kfi.loop_words
        min_common = int(F32(max_common) * F32(0.8))
        score_and_match = []
        for kfi in sharing:
            if kfi.loop_words > min_common:
                si = F32(score(bow, kfi.bow))
                kfi.loop_score = si
                if trace is not None:
                    trace["scored"].append(kfi.id)
                if si >= minScore:
                    score_and_match.append((si, kfi))
        if trace is not None:
            trace["passed"] = [k.id for _, k in score_and_match]
            trace["min_common"] = min_common
        if not score_and_match:
            return []
        acc_and_match = []
        best_acc = minScore
        for si, kfi in score_and_match:
            best_score, acc, best_kf = si, si, kfi
            for k2id in best_covisibles(kfi.id):
                kf2 = self.kfs.get(k2id)
                if kf2 is None:
                    continue
                if kf2.loop_query == qid and kf2.loop_words > min_common:
                    acc = F32(acc + kf2.loop_score)
                    if kf2.loop_score > best_score:
                        best_kf, best_score = kf2, kf2.loop_score
            acc_and_match.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        return self._retain(acc_and_match, best_acc, trace)

    def detect_relocalization_candidates(self, bow, best_covisibles, trace=None):   # :199-309
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
        if trace is not None:
            trace.update(sharing=[k.id for k in sharing], scored=[], passed=[], acc=[])
        if not sharing:
            return []
        max_common = 0
        for kfi in sharing:
            if kfi.reloc_words > max_common:
                max_common = kfi.reloc_words
        min_common = int(F32(max_common) * F32(0.8))
        score_and_match = []
        for kfi in sharing:
            if kfi.reloc_words > min_common:
                si = F32(score(bow, kfi.bow))
                kfi.reloc_score = si
                score_and_match.append((si, kfi))
        if trace is not None:
            trace["scored"] = trace["passed"] = [k.id for _, k in score_and_match]
            trace["min_common"] = min_common
        if not score_and_match:
            return []
        acc_and_match = []
        best_acc = F32(0)
        for si, kfi in score_and_match:
            best_score, acc, best_kf = si, si, kfi
            for k2id in best_covisibles(kfi.id):
                kf2 = self.kfs.get(k2id)
                if kf2 is None or kf2.reloc_query != qid:
                    continue
                acc = F32(acc + kf2.reloc_score)
                if kf2.reloc_score > best_score:
                    best_kf, best_score = kf2, kf2.reloc_score
            acc_and_match.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        return self._retain(acc_and_match, best_acc, trace)

    @staticmethod
    def _retain(acc_and_match, best_acc, trace):
        min_retain = F32(0.75) * best_acc
        if trace is not None:
            trace["acc"] = [(float(a), k.id) for a, k in acc_and_match]
            trace["min_retain"] = float(min_retain)
        out, seen = [], set()
        for acc, kf in acc_and_match:
            if acc > min_retain:
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
