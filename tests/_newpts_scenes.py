"""Scenes for the neighbour loop of CreateNewMapPoints in one call (afv_table_create_new_points).  TEST INFRASTRUCTURE ONLY.

The World scenes of tests/_tri_scenes.py cannot show that the chain works: every neighbour sees every point, so neighbour 0 takes them all
and neither the running id nor the hand-over of the masks is exercised.  A Chain wraps a World with STARTING MASKS that spread the points
over the neighbours:

    has_mp_nb[k][j] = 0  iff  j % nn == k  or  (j + 1) % nn == k      (feature j of neighbour k is free for two neighbours only)
    has_mp_cur[i]   = 1  iff  i % 7 == 3

th_low is 60.0 for binary rows and 1.0 for float rows.  ROWS lists the scenes with what the composed restatement (tests/_tri_ref.py
create_new_map_points over tests/_bow_ref.py search_for_triangulation) gives for them; tests/test_newpts_ref_cpu.py pins those figures, so
a scene that stops exercising the chain fails on the CPU.
"""
import numpy as np

import _tri_ref as R
import _tri_scenes as S

# (seed, nn, n, desc_bytes, float_dim) -> new points per neighbour, the stale-mask batch's total
ROWS = {
    (1, 3, 40, 32, 0): ((23, 11, 0), 68),
    (2, 7, 70, 32, 0): ((20, 10, 10, 0, 10, 10, 0), 119),
    (3, 20, 130, 32, 0): ((11, 6, 6, 6, 6, 6, 6, 6, 5, 7, 5, 5, 4, 4, 4, 4, 5, 5, 4, 0), 204),
    (5, 3, 257, 32, 0): ((146, 74, 0), 440),
    (6, 4, 64, 61, 0): ((27, 14, 14, 0), 110),
    (7, 3, 48, 0, 128): ((27, 14, 0), 82),
}


class Chain:
    """a World, its starting masks and the restatement's answer: want = [(id, k, i, j, fields)] in creation order"""

    def __init__(self, seed, nn, n, desc_bytes=32, float_dim=0, first_id=4):
        self.key = (seed, nn, n, desc_bytes, float_dim)
        self.W = S.World(seed, nn=nn, n=n, desc_bytes=desc_bytes or 32, float_dim=float_dim)
        self.nn, self.n, self.desc_bytes, self.float_dim, self.first_id = nn, n, desc_bytes or 32, float_dim, first_id
        self.th_low = 1.0 if float_dim else 60.0
        j = np.arange(n)
        self.has_mp_nb = [(~((j % nn == k) | ((j + 1) % nn == k))).astype(np.uint8) for k in range(nn)]
        self.has_mp_cur = (j % 7 == 3).astype(np.uint8)
        self._want = {}

    def masks(self):
        """fresh copies of the starting masks: (cur, [per neighbour])"""
        return self.has_mp_cur.copy(), [m.copy() for m in self.has_mp_nb]

    def restate(self, has_mp_cur=None, has_mp_nb=None, first_id=None):
        cur, nb = self.masks()
        W = self.W
        return R.create_new_map_points(W.kfs[0], W.kfs[1:], W.jobs, W.search(self.th_low), cur if has_mp_cur is None else has_mp_cur,
                                       nb if has_mp_nb is None else has_mp_nb, first_id=self.first_id if first_id is None else first_id)

    @property
    def want(self):
        if "chain" not in self._want:
            self._want["chain"] = self.restate()
        return self._want["chain"]

    def per_neighbour(self, want=None):
        want = self.want if want is None else want
        return tuple(sum(1 for w in want if w[1] == k) for k in range(self.nn))

    def final_masks(self, want=None, start=None):
        """the masks after the loop: the starting ones plus every accepted (i, j)"""
        cur, nb = self.masks() if start is None else (start[0].copy(), [m.copy() for m in start[1]])
        for _, k, i, j, _ in (self.want if want is None else want):
            cur[i] = 1
            nb[k][j] = 1
        return cur, nb

    def stale_total(self):
        """every neighbour searched under the STARTING masks (one batched call): the total the chain must not give"""
        W = self.W
        search = W.search(self.th_low)
        total = 0
        for k in range(self.nn):
            m = np.asarray(search(k, self.has_mp_cur, self.has_mp_nb[k]), np.int32)
            total += sum(1 for i in range(W.n) if R.triangulate_match(W.jobs[k], W.kfs[0], i, W.kfs[k + 1], int(m[i]))[0] == R.ACCEPTED)
        return total


_CHAINS = {}


def chain(*key):
    """Chain(seed, nn, n, desc_bytes, float_dim), built once per process and never changed"""
    if key not in _CHAINS:
        _CHAINS[key] = Chain(*key)
    return _CHAINS[key]
