"""Constructed scenes for afv_table_refresh_points (tests/_refresh_ref.py is the semantics).  TEST INFRASTRUCTURE ONLY.

A scene is a keyframe table (rows, sigma2 and size planes per slot), the camera centres, a map-point store and one call: point ids, their
mpRefKF and their observations in the reference's order.  rule_scene(kind) holds one point per rule, named after the rule it reaches
(RULES); tests/test_refresh_ref_cpu.py proves that each reaches it.  sized_scene(kind, ...) holds points of given observation counts with
random rows.  kind = ("bytes", desc_bytes) or ("float", float_dim).

Rows "on a line": the row at t has its first t bits set (binary) or t in its first coordinate (float), so the distance of two rows grows
with |t_i - t_j| in both kinds and one construction serves all four tables.
"""
import numpy as np

from _refresh_ref import BAD, OBSERVED, SET

f32 = np.float32
KINDS = (("bytes", 32), ("bytes", 61), ("float", 128), ("float", 36))
KIND_IDS = ["bytes32", "bytes61", "float128", "float36"]
RULES = ("n1", "n2_identical_rows", "n3", "n4", "equal_medians", "bad_kf_front", "bad_kf_middle", "bad_kf_end", "all_kfs_bad", "point_bad",
         "point_unset", "r1_ref_minus_one", "r1_ref_not_observing", "r2_zero_distance", "r2_not_finite", "ref_differs_from_chosen",
         "no_observations")
ONLY = {"pad_bytes_differ": ("bytes", 61), "float_equal_distances": ("float", None)}


class Scene:
    def __init__(self, kind, nslots, cap, seed):
        self.kind = kind
        self.float_dim = kind[1] if kind[0] == "float" else 0
        self.desc_bytes = 4 * kind[1] if self.float_dim else kind[1]
        self.pitch = self.desc_bytes if self.float_dim else (32 if self.desc_bytes <= 32 else 64)
        self.nslots, self.cap = nslots, cap
        rng = np.random.RandomState(seed)
        self.rng = rng
        self.kfs = list(range(nslots))
        if self.float_dim:
            self.rows = {s: rng.rand(cap, self.float_dim).astype(np.float32) for s in self.kfs}
        else:
            self.rows = {s: rng.randint(0, 256, (cap, self.pitch)).astype(np.uint8) for s in self.kfs}
            for s in self.kfs:
                self.rows[s][:, self.desc_bytes:] = 0
        self.sigma2 = {s: (f32(1.2) ** rng.randint(0, 8, cap)).astype(np.float32) ** 2 for s in self.kfs}
        self.size = {s: (f32(31.0) * f32(1.2) ** rng.randint(0, 8, cap)).astype(np.float32) for s in self.kfs}
        self.x = {s: (rng.rand(cap) * 90).astype(np.float32) for s in self.kfs}
        self.y = {s: (rng.rand(cap) * 60).astype(np.float32) for s in self.kfs}
        self.centres = {s: (rng.randn(3) * 2).astype(np.float32) for s in self.kfs}
        self.max_size = {s: f32(31.0) * f32(1.2) ** 7 for s in self.kfs}
        self.kf_bad = []
        self.store, self.point_ids, self.ref_kf, self.observations, self.rule = {}, [], {}, [], {}

    # ---- rows ----
    def line_row(self, t):
        if self.float_dim:
            r = np.zeros(self.float_dim, np.float32)
            r[0] = t
            return r
        r = np.zeros(self.pitch, np.uint8)
        r[:t // 8] = 255
        if t % 8:
            r[t // 8] = (1 << (t % 8)) - 1
        return r

    def set_row(self, slot, idx, row):
        self.rows[slot][idx] = row

    def table_rows(self, slot):
        """what DescriptorTable.set takes: desc_bytes wide (the pad bytes stay behind)"""
        return self.rows[slot] if self.float_dim else np.ascontiguousarray(self.rows[slot][:, :self.desc_bytes])

    # ---- points ----
    def stored(self, pid, pos=None, flags=SET | OBSERVED):
        rng = self.rng
        width = self.float_dim if self.float_dim else self.desc_bytes
        self.store[pid] = {
            "pos": (rng.randn(3) * 3 + np.array([0, 0, 12])).astype(np.float32) if pos is None else np.asarray(pos, np.float32),
            "normal": rng.randn(3).astype(np.float32), "min_distance": f32(rng.rand() + 1), "max_distance": f32(rng.rand() + 20),
            "ref_size": f32(31.0), "ref_distance": f32(rng.rand() + 5), "ref_sigma": f32(1.0), "flags": np.uint8(flags),
            "descriptors": rng.rand(width).astype(np.float32) if self.float_dim else rng.randint(0, 256, width).astype(np.uint8)}

    def point(self, pid, obs, ref, rule=None, **kw):
        """obs [(slot, idx), ...] in list order; ref: the slot of mpRefKF | None"""
        self.stored(pid, **kw)
        self.point_ids.append(pid)
        if ref is not None:
            self.ref_kf[pid] = ref
        self.observations += [(pid, s, i) for s, i in obs]
        if rule:
            self.rule[rule] = pid

    def store_arrays(self, ids):
        out = {k: np.array([self.store[i][k] for i in ids]) for k in ("pos", "normal", "min_distance", "max_distance", "ref_size", "ref_distance",
                                                                     "ref_sigma", "flags", "descriptors")}
        return out


def edge_arrays(sc):
    """the observation arrays of the C call: grouped by point in the order of point_ids, a stable sort; order[e] = the observation edge e
    came from"""
    where_p, where_k = {p: i for i, p in enumerate(sc.point_ids)}, {s: i for i, s in enumerate(sc.kfs)}
    pk = np.array([(where_p[p], where_k[s], i) for p, s, i in sc.observations], np.int32).reshape(-1, 3)
    order = np.argsort(pk[:, 0], kind="stable")
    pk = pk[order]
    return np.ascontiguousarray(pk[:, 0]), np.ascontiguousarray(pk[:, 1]), np.ascontiguousarray(pk[:, 2]), order


def rule_scene(kind, seed=7):
    """one point per rule; the ids 100 .. are in the store but not named in the call"""
    S = Scene(kind, nslots=8, cap=24, seed=seed)
    nxt = [0]

    def line(ts, slots=None):
        """a fresh feature index per row: rows at ts in the slots 0, 1, ... -> obs"""
        idx = nxt[0]
        nxt[0] += 1
        slots = list(range(len(ts))) if slots is None else slots
        for s, t in zip(slots, ts):
            S.set_row(s, idx, S.line_row(t))
        return [(s, idx) for s in slots]

    S.point(0, line([5]), 0, "n1")
    S.point(1, line([3, 3]), 1, "n2_identical_rows")
    S.point(2, line([0, 5, 7]), 0, "n3")            # medians 5, 2, 2: row 1
    S.point(3, line([0, 9, 10, 30]), 2, "n4")       # m = 1: medians 9, 1, 1, 20: row 1
    S.point(4, line([0, 1, 10, 11]), 0, "equal_medians")  # all 1: row 0
    # the bad keyframe's row would win if it were counted: rows at 10, 10, 10 and the others far apart
    S.kf_bad = [5, 6, 7]
    S.point(5, line([10, 10, 0, 30, 10], [5, 0, 1, 2, 6]), 0, "bad_kf_front")
    S.point(6, line([0, 10, 10, 10, 30], [0, 5, 6, 7, 1]), 1, "bad_kf_middle")
    S.point(7, line([0, 30, 10, 10], [0, 1, 5, 6]), 0, "bad_kf_end")
    S.point(8, line([1, 2, 3], [5, 6, 7]), 6, "all_kfs_bad")
    S.point(9, line([1, 2, 3]), 0, "point_bad", flags=SET | BAD | OBSERVED)
    S.point(10, line([1, 2, 3]), 0, "point_unset", flags=0)
    S.point(11, line([1, 2, 3]), None, "r1_ref_minus_one")
    S.point(12, line([1, 2, 3]), 4, "r1_ref_not_observing")
    S.point(13, line([1, 2, 3]), 0, "r2_zero_distance", pos=S.centres[1])
    S.point(14, line([1, 2, 3]), 0, "r2_not_finite", pos=[np.inf, 0.0, 1.0])
    S.point(15, line([4, 4, 20]), 2, "ref_differs_from_chosen")  # row 0 is chosen, mpRefKF is slot 2
    S.point(16, [], 0, "no_observations")
    if kind == ("bytes", 61):
        # without the pad bytes rows 0 and 1 are identical and row 0 wins; counted, the pads would push rows 0, 1 apart and row 1 would win
        obs = line([8, 8, 9, 40])
        idx = obs[0][1]
        S.rows[0][idx, 61:] = 255
        S.rows[2][idx, 61:] = 0
        S.rows[3][idx, 61:] = 0x0f
        S.point(17, obs, 0, "pad_bytes_differ")
    if kind[0] == "float":
        idx = nxt[0]
        nxt[0] += 1
        for s in range(3):  # one-hot rows: every distance is 2
            r = np.zeros(S.float_dim, np.float32)
            r[s + 1] = 1.0
            S.set_row(s, idx, r)
        S.point(17, [(s, idx) for s in range(3)], 1, "float_equal_distances")
    for pid in (100, 101, 102):
        S.stored(pid)
    return S


def sized_scene(kind, counts, seed=11, cap=6):
    """point p has counts[p] observations, in the slots 0 .. counts[p] - 1, random rows; every fourth keyframe of a long list is bad"""
    nslots = max(max(counts), 1)
    S = Scene(kind, nslots=nslots, cap=cap, seed=seed)
    rng = S.rng
    if nslots > 8:
        S.kf_bad = [s for s in range(nslots) if s % 4 == 3]
    for p, n in enumerate(counts):
        obs = [(s, int(rng.randint(cap))) for s in range(n)]
        S.point(p, obs, int(rng.randint(n)) if n else None)
    S.stored(len(counts))  # one id the call does not name
    return S
