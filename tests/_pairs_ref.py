"""Plain-Python restatement of the two-phase brute-force pair matcher (csrc/k_match.hip, csrc/k_match_mfma.hip).  TEST INFRASTRUCTURE ONLY.

Phase 1 leaves ONE RECORD per row: seven key slots + nk, the length of the exact prefix.  Phase 2 decides every row from its record and the
columns taken by the rows before it, and rescans the free columns exactly where the record is used up.  Restated here from the COMMENTS
of the kernels (what a record means), not from their code paths:

  hamming, key                 key = distance << 16 | column, NO_KEY = 0x7fffffff; a row's exact order is ascending key
  records_popcount             k_match_topk: the four smallest keys, slots 4..6 NO_KEY, nk = 4
  records_mfma                 k_match_topk_mfma, unsliced: column c belongs to lane half (c % 8) // 4, each half keeps its four smallest
                               keys, the record is the first seven of the merged eight, nk = the number of them <= t = the smaller of the
                               halves' fourth keys (7 when t == NO_KEY: a half with fewer than four columns has no fourth key)
  records_sliced               the same, the 64-column tiles dealt ceil(ntiles / nslices) per slice: per-slice records and their merge
                               under `bound`
  record_contract              what ANY engine's record must satisfy, whatever its internals
  resolve_model                the sequential meaning of phase 2 on given records, with a class per row (CLASSES)

The outcome is not restated again: FeatureMatcher.cc:587-641 is tests/_bow_ref.py's search_by_bow_kf_kf (no nodes) and the rotation
histogram is _bow_ref's / _proj_ref's; tests/test_pairs_ref_cpu.py holds resolve_model + histogram to both and to the oracle binding.

`flip="rule"` turns ONE rule around (FLIPS).  A RECORD flip changes what phase 1 writes and must break record_contract; an OUTCOME flip
changes phase 2 and must change the answer of the scene that sits on it; a TRACE flip is one of the four shortcuts whose only effect is
which rows are looked at or rescanned - no valid record can make the answer differ (that is why the kernels may take them), so the scene
proves it sits on the rule by the class of its named row changing (FLIP_KIND).
"""
import numpy as np

from _bow_ref import HISTO_LENGTH, rotation_bin, three_maxima

f32 = np.float32
NO_KEY = 0x7fffffff
RKEYS = 7
FLT_MAX = np.finfo(np.float32).max
_POP = np.array([bin(i).count("1") for i in range(256)], np.uint16)

CLASSES = ("dead", "keys_accept", "keys_reject", "best_fails_th", "bound_accept", "rescan_take", "rescan_none", "nokey_bound_fail",
           "complete_list")

# rule -> what the flipped restatement does instead
FLIPS = {
    "nk_plus1": "phase 1 writes nk + 1 (at most 7): one key more than is exact counts as exact",
    "tail_exact": "phase 2 reads all seven slots as exact, whatever nk says",
    "bound_le": "exhausted, best < ratio * last_d accepts  ->  <= accepts (a column outside the list may sit exactly at last_d)",
    "guard_dropped": "exhausted AND n2 > nk  ->  exhausted alone: a list that holds every column is treated as used up",
    "nokey_le": "no key left: last_d < th rescans  ->  last_d <= th rescans (last_d == th: the refusal becomes a rescan that finds nothing)",
    "rescan_sees_taken": "the exact rescan runs over the FREE columns  ->  over all of them",
    "rescan_tie_high": "of two free columns at the best distance the rescan takes the lower  ->  the higher",
    "complete_ignored": "a NO_KEY inside the exact prefix ends the list (`complete`)  ->  it does not",
    "slice_bound": "bound = min over the slices whose exact prefix holds no NO_KEY of their last exact key  ->  those slices are ignored: no bound",
    "dead_kept_live": "a row whose first key fails (float)d < th is dead (never looked at again)  ->  it stays live",
}
FLIP_KIND = {"nk_plus1": "record", "slice_bound": "record", "tail_exact": "outcome", "bound_le": "outcome", "rescan_sees_taken": "outcome",
             "rescan_tie_high": "outcome", "guard_dropped": "trace", "nokey_le": "trace", "complete_ignored": "trace", "dead_kept_live": "trace"}
assert set(FLIP_KIND) == set(FLIPS)


# ---- a) distances and keys ----
def hamming(D1, D2):
    """[n1, n2] int32 over the stored bytes"""
    D1, D2 = np.ascontiguousarray(D1, np.uint8), np.ascontiguousarray(D2, np.uint8)
    out = np.zeros((len(D1), len(D2)), np.int32)
    for i in range(len(D1)):
        out[i] = _POP[D1[i][None, :] ^ D2].sum(1) if len(D2) else 0
    return out


def key_of(d, c):
    return (int(d) << 16) | int(c)


def row_keys(dist_row, cols=None):
    """every key of a row, ascending: distance first, then column.  cols: the column indices dist_row ranges over (default 0 .. n2 - 1)"""
    d = np.asarray(dist_row, np.int64)
    c = np.arange(len(d), dtype=np.int64) if cols is None else np.asarray(cols, np.int64)
    return np.sort((d << 16) | c)


def _pad(keys, n):
    out = np.full(n, NO_KEY, np.int64)
    out[:min(len(keys), n)] = keys[:n]
    return out


# ---- b) record models: [n1][8] int32, slots 0..6 + nk ----
def _rec_popcount(dist_row):
    rec = np.full(8, NO_KEY, np.int64)
    rec[:4] = _pad(row_keys(dist_row), 4)
    rec[7] = 4
    return rec


def _rec_mfma(dist_row, cols):
    """one row over the columns `cols` (absolute indices; the lane half of a column is a property of its absolute index: tiles start at
    multiples of 64)"""
    cols = np.asarray(cols, np.int64)
    d = np.asarray(dist_row, np.int64)
    half = (cols % 8) // 4
    tops = [_pad(row_keys(d[half == h], cols[half == h]), 4) for h in (0, 1)]
    t = int(min(tops[0][3], tops[1][3]))
    kept = np.sort(np.concatenate(tops))[:RKEYS]
    rec = np.full(8, NO_KEY, np.int64)
    rec[:RKEYS] = kept
    rec[7] = RKEYS if t == NO_KEY else int(np.sum((kept != NO_KEY) & (kept <= t)))
    return rec


def _bump(rec, flip):
    if flip == "nk_plus1":
        rec[7] = min(int(rec[7]) + 1, RKEYS)
    return rec


def records_popcount(dist, flip=None):
    return np.stack([_bump(_rec_popcount(r), flip) for r in dist]).astype(np.int32) if len(dist) else np.zeros((0, 8), np.int32)


def records_mfma(dist, flip=None):
    n2 = dist.shape[1]
    return (np.stack([_bump(_rec_mfma(r, np.arange(n2)), flip) for r in dist]).astype(np.int32) if len(dist)
            else np.zeros((0, 8), np.int32))


def topk_slices(cap, engine):
    """afv_match_topk_slices(cap, engine, ((cap + 63) // 64 + 1) // 2): the popcount engine never slices"""
    want = ((cap + 63) // 64 + 1) // 2
    return max(1, min(want, 16)) if (engine == 1 and cap < 8192) else 1


def slice_columns(n2, nslices):
    """the column range of every slice: the 64-column tiles dealt ceil(ntiles / nslices) per slice"""
    ntiles = (n2 + 63) // 64
    per = (ntiles + nslices - 1) // nslices
    out = []
    for s in range(nslices):
        t0, t1 = s * per, min((s + 1) * per, ntiles)
        out.append(np.arange(min(t0 * 64, n2), min(max(t1, t0) * 64, n2)) if t0 < t1 else np.zeros(0, np.int64))
    return out


def records_sliced(dist, nslices, flip=None):
    """(merged [n1][8], per slice [n1][nslices][8])"""
    n1, n2 = dist.shape
    sl = slice_columns(n2, nslices)
    per = np.full((n1, nslices, 8), NO_KEY, np.int64)
    merged = np.full((n1, 8), NO_KEY, np.int64)
    for i in range(n1):
        bound = NO_KEY
        for s, cols in enumerate(sl):
            r = _rec_mfma(dist[i, cols], cols)     # (an empty slice: all NO_KEY, t == NO_KEY, nk = 7)
            per[i, s] = r
            nk = int(r[7])
            bounds = not np.any(r[:nk] == NO_KEY)         # its exact prefix holds no NO_KEY: the slice has columns outside it
            if bounds and flip != "slice_bound":
                bound = min(bound, int(r[nk - 1]))
        kept = np.sort(per[i, :, :RKEYS].reshape(-1))[:RKEYS]
        merged[i, :RKEYS] = kept
        merged[i, 7] = RKEYS if bound == NO_KEY else int(np.sum((kept != NO_KEY) & (kept <= bound)))
        _bump(merged[i], flip)
    return merged.astype(np.int32), per.astype(np.int32)


def records(model, dist, cap=320, flip=None):
    """model: "popcount" | "mfma" | "sliced" """
    if model == "popcount":
        return records_popcount(dist, flip)
    if model == "mfma":
        return records_mfma(dist, flip)
    return records_sliced(dist, topk_slices(cap, 1), flip)[0]


MODELS = ("popcount", "mfma", "sliced")


# ---- c) what any record must satisfy ----
def record_contract(rec, dist_row, n2, cols=None):
    """None when `rec` (8 ints) is a valid record of a row with distances dist_row to its n2 columns, else a sentence saying what is wrong.
    cols: the absolute indices of those columns (a slice's record ranges over its own)"""
    rec = [int(v) for v in rec]
    nk = rec[7]
    if not 1 <= nk <= RKEYS:
        return "nk = %d outside 1..7" % nk
    if nk < min(4, n2):
        return "nk = %d < min(4, n2 = %d)" % (nk, n2)
    exact = row_keys(dist_row, cols)
    assert len(exact) == n2
    want = [int(v) for v in _pad(exact, nk)]
    if rec[:nk] != want:
        return "slots [0, %d) are %s, the row's nearest are %s" % (nk, rec[:nk], want)
    real = set(int(v) for v in exact)
    for q in range(nk, RKEYS):
        if rec[q] != NO_KEY and rec[q] not in real:
            return "slot %d holds %#x: not the key of a column of this row" % (q, rec[q])
    listed = [k for k in rec[:RKEYS] if k != NO_KEY]
    if any(b <= a for a, b in zip(listed, listed[1:])):
        return "slots not strictly ascending: %s" % listed
    if any(rec[q] == NO_KEY and rec[q + 1] != NO_KEY for q in range(RKEYS - 1)):
        return "a key behind a NO_KEY slot: %s" % rec[:RKEYS]
    return None


# ---- d) phase 2, sequentially ----
def _flipset(flip):
    """one rule or several at once (a set): two of the shortcuts cover for each other and only show when both are turned"""
    fl = set() if flip is None else ({flip} if isinstance(flip, str) else set(flip))
    assert fl <= set(FLIPS), fl
    return fl


def _rescan(dist_row, taken, th, ratio, flip):
    """the exact (best key, second distance) over the free columns -> the column taken or -1"""
    free = np.ones(len(dist_row), bool) if "rescan_sees_taken" in flip else ~taken
    idx = np.nonzero(free)[0]
    if not len(idx):
        return -1
    d = dist_row[idx]
    order = np.lexsort((-idx, d)) if "rescan_tie_high" in flip else np.lexsort((idx, d))
    best = int(idx[order[0]])
    best1 = f32(dist_row[best])
    best2 = FLT_MAX if len(order) < 2 else f32(d[order[1]])
    return best if (best1 < th and best1 < f32(ratio) * best2) else -1


def resolve_model(recs, dist, n2, th, ratio, flip=None):
    """(match [n1], count, trace) - before the rotation histogram.  trace: cls[n1] the class of every row, slot[n1] its live slot (-1: dead),
    nk[n1] the prefix length phase 2 used, rescans = rows that needed the exact rescan"""
    n1 = len(recs)
    flip = _flipset(flip)
    th, ratio = f32(th), f32(ratio)
    dist = np.asarray(dist)
    out = np.full(n1, -1, np.int32)
    taken = np.zeros(n2, bool)
    tr = {"cls": [None] * n1, "slot": np.full(n1, -1, np.int64), "nk": np.zeros(n1, np.int64), "rescans": []}
    nlive = nm = 0
    for i in range(n1):
        keys = [int(v) for v in recs[i][:RKEYS]]
        nk = RKEYS if "tail_exact" in flip else min(max(int(recs[i][7]), 1), RKEYS)
        tr["nk"][i] = nk
        if not (keys[0] != NO_KEY and f32(keys[0] >> 16) < th):
            tr["cls"][i] = "dead"
            if "dead_kept_live" not in flip:
                continue
        tr["slot"][i] = nlive
        nlive += 1
        last_d = f32(keys[nk - 1] >> 16)          # every column outside the list is at least this far
        complete = any(k == NO_KEY for k in keys[:nk]) and "complete_ignored" not in flip
        free = [k for k in keys[:nk] if k != NO_KEY and not taken[k & 0xffff]]
        best = free[0] if free else None
        second = free[1] if len(free) > 1 else None
        exhausted = second is None and not complete
        want, cls, rescan = -1, None, False
        if best is not None and not f32(best >> 16) < th:
            cls = "best_fails_th"
        elif exhausted and (n2 > nk or "guard_dropped" in flip):
            if best is not None:
                b1, lim = f32(best >> 16), ratio * last_d
                if (b1 <= lim) if "bound_le" in flip else (b1 < lim):
                    want, cls = best & 0xffff, "bound_accept"
                else:
                    rescan = True
            elif (last_d <= th) if "nokey_le" in flip else (last_d < th):
                rescan = True
            else:
                cls = "nokey_bound_fail"
        elif best is not None:
            b1 = f32(best >> 16)
            b2 = FLT_MAX if second is None else f32(second >> 16)
            ok = bool(b1 < th and b1 < ratio * b2)
            want = (best & 0xffff) if ok else -1
            cls = "complete_list" if second is None else ("keys_accept" if ok else "keys_reject")
        else:
            cls = "complete_list"
        if rescan:
            tr["rescans"].append(i)
            want = _rescan(dist[i], taken, th, ratio, flip)
            cls = "rescan_take" if want >= 0 else "rescan_none"
        if tr["cls"][i] is None:
            tr["cls"][i] = cls
        if want >= 0:
            out[i] = want
            taken[want] = True
            nm += 1
    return out, nm, tr


def rotation_filter(match, nm, angle1, angle2):
    """FeatureMatcher.cc:1587-1668 on a match vector, keyed by the row (:638): _bow_ref's bins and maxima"""
    match = match.copy()
    tr = {"eq": {k: 0 for k in ("rot_lt0", "rot_round", "rot_wrap", "max_first", "max2_lt", "max3_lt")}, "wraps": 0, "rule01": 0}
    hist = [[] for _ in range(HISTO_LENGTH)]
    for i, c in enumerate(match):
        if c >= 0:
            hist[rotation_bin(angle1[i], angle2[c], tr, None)].append(i)
    keep = three_maxima([len(h) for h in hist], tr, None)
    for b in range(HISTO_LENGTH):
        if b not in keep:
            for i in hist[b]:
                match[i] = -1
                nm -= 1
    return match, nm


def match_pair(model, D1, D2, th, ratio, check_orientation=False, angle1=None, angle2=None, cap=320, flip=None, dist=None):
    """phase 1 (`model`) + phase 2 + the histogram: (match, count, trace, records)"""
    dist = hamming(D1, D2) if dist is None else dist
    fl = _flipset(flip)
    rec_flip = [f for f in fl if FLIP_KIND[f] == "record"]
    assert len(rec_flip) <= 1
    recs = records(model, dist, cap, rec_flip[0] if rec_flip else None)
    m, nm, tr = resolve_model(recs, dist, dist.shape[1], th, ratio, fl - set(rec_flip))
    if check_orientation:
        m, nm = rotation_filter(m, nm, angle1, angle2)
    return m, nm, tr, recs
