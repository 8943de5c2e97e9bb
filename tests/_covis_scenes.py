"""Constructed scenes for the covisibility count and the local map (tests/_covis_ref.py is the restatement they are answered by).

A scene is a dict: cap / nsets (the table), planes {slot: [ids]}, capacity / set / bad (the store), slots / key_ids / kf_bad (the listed
keyframes), queries (dicts as covisibility.covisibility_votes takes them), local / frame_pts (the local-points call), and `variant`: the wrong
reading of the restatement the scene is built to tell apart (None: a sweep scene).  answer(scene) is what every route must give.
"""
import numpy as np

import _covis_ref as R


def _scene(name, planes, capacity, set_ids, bad=(), slots=None, key_ids=None, kf_bad=None, queries=(), local=None, frame_pts=None, variant=None,
           cap=None, nsets=None):
    planes = {int(s): [int(i) for i in p] for s, p in planes.items()}
    slots = sorted(planes) if slots is None else list(slots)
    return {"name": name, "planes": planes, "capacity": int(capacity), "set": sorted(set(int(i) for i in set_ids)), "bad": sorted(set(int(i) for i in bad)),
            "slots": slots, "key_ids": list(range(len(slots))) if key_ids is None else list(key_ids), "kf_bad": kf_bad, "queries": list(queries),
            "local": local, "frame_pts": frame_pts, "variant": variant, "cap": cap or max([len(p) for p in planes.values()] + [1]),
            "nsets": nsets or (max(planes) + 1)}


def answer(sc, wrong=None):
    store = R.Store(sc["capacity"], sc["set"], sc["bad"])
    out = {}
    if sc["queries"]:
        qs = [("slot", q["slot"]) if "slot" in q else ("ids", q["ids"]) for q in sc["queries"]]
        votes = R.votes(sc["planes"], store, sc["slots"], qs, wrong)
        order, best, nz = [], [], []
        for q, row in zip(sc["queries"], votes):
            o, b, n = R.connect(row, sc["key_ids"], q.get("th", 15), q.get("skip_bad", False), sc["kf_bad"], wrong)
            order.append(o); best.append(b); nz.append(n)
        out.update(votes=votes, order=order, best=best, nz=nz)
    if sc["local"] is not None:
        ids, seen = R.local_points(sc["planes"], store, sc["local"], sc["frame_pts"], wrong)
        out.update(local_ids=ids, seen=seen)
    return out


# ---- the scenes named after a rule ----
def q_duplicate():
    """id 5 stands twice in Q: the reference loops over pts, it counts twice"""
    return _scene("q_duplicate", {0: [5, 6, 7], 1: [5, 9]}, 16, range(16), queries=[{"ids": [5, 5, 6, -1], "th": 1}], variant="q_dup_once")


def plane_duplicate():
    """id 5 stands at two features of slot 1: the observations are a map, it counts once"""
    return _scene("plane_duplicate", {0: [5, 6], 1: [5, 5, 6, 8]}, 16, range(16), queries=[{"slot": 0, "th": 1}, {"ids": [5], "th": 1}],
                  variant="plane_dup_twice")


def self_excluded():
    return _scene("self_excluded", {0: [1, 2, 3], 1: [1, 2], 2: [3]}, 8, range(8), queries=[{"slot": 0, "th": 1}, {"slot": 1, "th": 1}],
                  variant="self_counted")


def order_ties():
    """slots 1 and 2 tie at 16 votes at th 15, slot 3 has 17: order by votes, then keyId DESCENDING; keyIds against the list order"""
    a = list(range(0, 16))
    return _scene("order_ties", {0: list(range(0, 20)), 1: a, 2: a, 3: list(range(0, 17)), 4: [0]}, 32, range(32), key_ids=[40, 7, 30, 9, 2],
                  queries=[{"slot": 0, "th": 15}], variant="ties_ascending")


def best_tie():
    """nobody at th 15, slots 1 and 2 tie at 3: best is the LOWEST keyId, and it alone is the order"""
    return _scene("best_tie", {0: [1, 2, 3, 4], 1: [1, 2, 3], 2: [2, 3, 4], 3: [4]}, 8, range(8), key_ids=[5, 9, 3, 1],
                  queries=[{"slot": 0, "th": 15}], variant="best_tie_highest")


def fallback():
    return _scene("fallback", {0: [1, 2, 3, 4], 1: [1, 2, 3], 2: [4]}, 8, range(8), queries=[{"slot": 0, "th": 15}], variant="no_fallback")


def th_edge():
    """votes of 14 and 15 against th 15"""
    return _scene("th_edge", {0: list(range(20)), 1: list(range(14)), 2: list(range(15)), 3: list(range(5, 20))}, 32, range(32),
                  queries=[{"slot": 0, "th": 15}, {"ids": list(range(15)), "th": 15}], variant="th_strict")


def skip_bad():
    """the bad keyframe (slot 1) has the most votes: it keeps them, but is neither best nor in the order"""
    return _scene("skip_bad", {0: [1, 2], 1: [1, 2, 3, 4], 2: [3], 3: [9]}, 16, range(16), kf_bad=[0, 1, 0, 0], key_ids=[3, 2, 1, 0],
                  queries=[{"ids": [1, 2, 3, 4, -1], "th": 1, "skip_bad": True}, {"ids": [1, 2, 3, 4], "th": 1}], variant="bad_kf_best")


def first_occurrence():
    """id 4 twice inside plane 2 and again in plane 0; id 7 in both planes: each at its first place in the walk 2, 0"""
    return _scene("first_occurrence", {0: [7, 4, 1, -1, 3], 2: [4, 9, 4, 7, 2]}, 16, range(16), bad=[9], local=[2, 0], frame_pts=[7, -1, 3, 9, 11],
                  variant="last_occurrence")


def all_zero():
    return _scene("all_zero", {0: [1, 2], 1: [3], 2: [-1, -1]}, 8, range(8), queries=[{"ids": [5, 6], "th": 1}, {"slot": 2, "th": 15}, {"ids": [], "th": 1}])


def good_filter():
    """-1, bad (3), never set (6) and the ends 0 and capacity - 1 on both sides"""
    return _scene("good_filter", {0: [0, 3, 6, 15, -1, 2], 1: [15, 3, 6, 0, 2, 2], 2: [3, 6, -1]}, 16, [0, 1, 2, 3, 15], bad=[3],
                  queries=[{"slot": 0, "th": 1}, {"ids": [0, 3, 6, 15, -1, 2, 1], "th": 1}, {"slot": 2, "th": 1}], local=[2, 1, 0], frame_pts=[3, 6, 0, -1, 15])


def hash_collisions():
    """plane ids that share their low 10 to 16 bits"""
    capacity = 1 << 20
    a = [(k << b) | 5 for b in (10, 12, 16) for k in range(1, 12)]
    b = a[::2] + [(k << 16) | 6 for k in range(1, 9)]
    return _scene("hash_collisions", {0: a, 1: b, 2: [x + 1 for x in a]}, capacity, set(a) | set(b) | set(x + 1 for x in a),
                  queries=[{"slot": 0, "th": 15}, {"slot": 1, "th": 1}, {"ids": a + b, "th": 15}], local=[0, 1, 2], frame_pts=b)


RULE_SCENES = (q_duplicate, plane_duplicate, self_excluded, order_ties, best_tie, fallback, th_edge, skip_bad, first_occurrence)
PLAIN_SCENES = (all_zero, good_filter, hash_collisions)


# ---- sweep scenes: seeded maps of a given shape ----
def random_scene(seed, counts, cap, capacity, nq_slot, id_lengths=(), pool=None, th=15, with_bad_kf=False, local=None, n_frame=0, shuffle_keys=True):
    """counts: features per slot.  Ids come from a pool small enough that keyframes share points; a tenth of the entries are -1, a few ids
    are bad or never set, ids 0 and capacity - 1 are in the pool."""
    rng = np.random.RandomState(seed)
    nk = len(counts)
    pool = pool or max(8, min(capacity, 3 * max(max(counts), 1)))
    ids = np.unique(np.concatenate([rng.randint(0, capacity, pool), [0, capacity - 1]]))
    never, bad = set(ids[rng.rand(len(ids)) < 0.05].tolist()), set(ids[rng.rand(len(ids)) < 0.05].tolist())
    planes = {}
    for s, n in enumerate(counts):
        p = ids[rng.randint(0, len(ids), n)].astype(np.int64)
        p[rng.rand(n) < 0.1] = -1
        planes[s] = p.tolist()
    slots = rng.permutation(nk).tolist()
    key_ids = (rng.permutation(nk) * 3 + 1).tolist() if shuffle_keys else list(range(nk))
    queries = [{"slot": int(p), "th": th} for p in rng.permutation(nk)[:nq_slot]]
    kf_bad = (rng.rand(nk) < 0.2).astype(np.uint8).tolist() if with_bad_kf else None
    for k, n in enumerate(id_lengths):
        q = ids[rng.randint(0, len(ids), n)].astype(np.int64)
        q[rng.rand(n) < 0.1] = -1
        queries.append({"ids": q.tolist(), "th": 1 if k % 2 else th, "skip_bad": bool(with_bad_kf and k % 2)})
    rng.shuffle(queries)
    frame_pts = None
    if n_frame:
        frame_pts = ids[rng.randint(0, len(ids), n_frame)].tolist()
    return _scene("random_%d" % seed, planes, capacity, set(ids.tolist()) - never, bad, slots=slots, key_ids=key_ids, kf_bad=kf_bad, queries=queries,
                  local=local, frame_pts=frame_pts, cap=cap, nsets=nk)


def survivors_scene(total, nl, cap=130):
    """a local map of nl slots whose survivors number exactly `total`: every id twice, in its plane and in the next one"""
    per = -(-total // max(nl, 1)) if nl else 0
    assert per * 2 <= cap or nl == 0
    planes, nxt = {}, 0
    for s in range(max(nl, 1)):
        mine = list(range(nxt, min(nxt + per, total)))
        nxt += len(mine)
        planes[s] = mine
    for s in range(max(nl, 1)):
        planes[s] = planes[s] + planes[(s + 1) % max(nl, 1)]
    return _scene("survivors_%d_%d" % (total, nl), planes, max(total, 1) + 3, range(total), local=list(range(nl)), frame_pts=list(range(0, total, 3)),
                  cap=cap, nsets=max(nl, 1))


def dense(sc):
    """the scene as the flat arrays a table and a store hold: planes [nsets, cap] (-1 behind a slot's features), n [nsets], flags [capacity]
    (bit 0 set, bit 1 bad)"""
    planes = np.full((sc["nsets"], sc["cap"]), -1, np.int32)
    n = np.zeros(sc["nsets"], np.int32)
    for s, p in sc["planes"].items():
        planes[s, :len(p)] = p
        n[s] = len(p)
    flags = np.zeros(sc["capacity"], np.uint8)
    flags[sc["set"]] |= 1
    flags[sc["bad"]] |= 3  # a bad point was set
    return planes, n, flags
