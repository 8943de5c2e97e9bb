"""Host-side mirror of the reference's KeyFrameDatabase (include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc:40-309) and of the minScore
loop in front of DetectLoopCandidates (src/LoopClosing.cc:137-157), over a keyframe table that holds the keyframes' BowVectors.

The reference walks a per-word inverted file to count the words each keyframe shares with the query and then calls Vocabulary::score per
surviving keyframe.  Here both numbers come from ONE afv_table_score_bow call over the resident BowVectors (DescriptorTable.score_bow);
what stays on the host is the reference's own float arithmetic - the 0.8f and 0.75f gates and the covisibility accumulation.  The
covisibility graph is the caller's: GetConnectedKeyFrames / GetBestCovisibilityKeyFrames(10) come in as arguments.

Order: the reference meets keyframes word by word (ascending) and, inside a word's list, in insertion order; a keyframe enters
lKFsSharingWords when it is first met.  That is the order (smallest shared word, add sequence), which the device returns as
`first_common`.

KeyFrame::mRelocScore outlives a query in the reference, and DetectRelocalizationCandidates adds it for every neighbour that shares a
word with the frame, scored in THIS query or not (KeyFrameDatabase.cc:273-276).  The mirror keeps that member per slot; a keyframe that
was never scored reads 0 (the reference leaves it uninitialised, KeyFrame.cc:40).
Plumbing and float expressions only: no descriptor arithmetic happens here."""
import numpy as np

F32 = np.float32


class KeyFrameDatabase:
    def __init__(self, table):
        self.table = table
        self._seq = {}          # slot -> add sequence
        self._next = 0
        self._reloc_score = {}  # slot -> KeyFrame::mRelocScore

    # ---- KeyFrameDatabase::add / erase / clear (:40-73) ----
    def add(self, slot):
        slot = int(slot)
        if not 0 <= slot < self.table.nsets:
            raise ValueError("KeyFrameDatabase.add: slot %d outside the table" % slot)
        if slot not in self._seq:
            self._seq[slot] = self._next
            self._next += 1

    def erase(self, slot):
        self._seq.pop(int(slot), None)

    def clear(self):
        self._seq.clear()

    def _mask(self, exclude=()):
        mask = np.zeros(self.table.nsets, np.uint8)
        for s in self._seq:
            mask[s] = 1
        for s in exclude:
            if 0 <= int(s) < self.table.nsets:   # an id outside the table names no keyframe here (a negative one must not wrap around)
                mask[int(s)] = 0
        return mask

    def _sharing(self, query, mask):
        common, score, first = self.table.score_bow([query], mask)
        common, score, first = common[0], score[0], first[0]
        sharing = [s for s in self._seq if mask[s] and common[s] > 0]
        sharing.sort(key=lambda s: (int(first[s]), self._seq[s]))
        return sharing, common, score

    # ---- KeyFrameDatabase::DetectRelocalizationCandidates (:199-309) ----
    def DetectRelocalizationCandidates(self, frame, best_covisibles):
        """frame: a frame.Frame after ComputeBoW (its resident BowVector is the query), a slot, or a (word, value) pair;
        best_covisibles(slot) -> slots: the caller's GetBestCovisibilityKeyFrames(10).  Returns the candidate slots in the reference's order"""
        sharing, common, score = self._sharing(frame, self._mask())
        if not sharing:
            return []
        max_common = max(int(common[s]) for s in sharing)
        min_common = int(F32(max_common) * F32(0.8))
        scored = []
        for s in sharing:
            if int(common[s]) > min_common:
                si = F32(score[s])
                self._reloc_score[s] = si
                scored.append((si, s))
        if not scored:
            return []
        in_query = set(sharing)
        acc_and_match = []
        best_acc = F32(0)
        for si, s in scored:
            best_score, acc, best_kf = si, si, s
            for k2 in best_covisibles(s):
                k2 = int(k2)
                if k2 not in in_query:
                    continue
                s2 = self._reloc_score.get(k2, F32(0))
                acc = F32(acc + s2)
                if s2 > best_score:
                    best_kf, best_score = k2, s2
            acc_and_match.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        return self._retain(acc_and_match, best_acc)

    # ---- KeyFrameDatabase::DetectLoopCandidates (:76-197) ----
    def DetectLoopCandidates(self, slot, minScore, connected, best_covisibles):
        """slot: the query keyframe; connected: its GetConnectedKeyFrames (never candidates); minScore: min_score_to_connected"""
        min_score = F32(minScore)
        sharing, common, score = self._sharing(int(slot), self._mask(connected))
        if not sharing:
            return []
        max_common = max(int(common[s]) for s in sharing)
        min_common = int(F32(max_common) * F32(0.8))
        loop_score = {}
        scored = []
        for s in sharing:
            if int(common[s]) > min_common:
                si = F32(score[s])
                loop_score[s] = si
                if si >= min_score:
                    scored.append((si, s))
        if not scored:
            return []
        acc_and_match = []
        best_acc = min_score
        for si, s in scored:
            best_score, acc, best_kf = si, si, s
            for k2 in best_covisibles(s):
                k2 = int(k2)
                if k2 in loop_score:  # mnLoopQuery == this query && mnLoopWords > minCommonWords
                    acc = F32(acc + loop_score[k2])
                    if loop_score[k2] > best_score:
                        best_kf, best_score = k2, loop_score[k2]
            acc_and_match.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        return self._retain(acc_and_match, best_acc)

    @staticmethod
    def _retain(acc_and_match, best_acc):
        min_retain = F32(0.75) * best_acc
        out, seen = [], set()
        for acc, kf in acc_and_match:
            if acc > min_retain and kf not in seen:
                out.append(kf)
                seen.add(kf)
        return out

    # ---- LoopClosing::DetectLoop, the reference score (LoopClosing.cc:142-155) ----
    def min_score_to_connected(self, slot, connected):
        """the lowest score between keyframe `slot` and its covisible keyframes `connected` (the caller leaves out the bad ones)"""
        connected = [int(s) for s in connected if 0 <= int(s) < self.table.nsets]   # ids outside the table: skipped, like the C++ mirror
        min_score = F32(1)
        if not connected:
            return min_score
        mask = np.zeros(self.table.nsets, np.uint8)
        mask[connected] = 1
        _, score, _ = self.table.score_bow([int(slot)], mask, want_first=False)
        for s in connected:
            sc = F32(score[0][s])
            if sc < min_score:
                min_score = sc
        return min_score
