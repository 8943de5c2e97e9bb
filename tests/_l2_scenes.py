"""Float L2^2 scenes that tell summation orders apart, and the wrong arithmetics as code.  TEST INFRASTRUCTURE ONLY.

The float rows of _match_scenes.py, _proj_scenes.py and _stereo_scenes.py have small integer distances: exact in any arithmetic.  Here
every scene is a DUEL: a query row and two candidate rows A and B whose normative distances are equal or one float ulp apart, so that
the order of A and B (equal, A nearer, B nearer) differs between the normative arithmetic and ONE named wrong arithmetic.  A route that
evaluates the distance the wrong way answers differently: tests/test_l2_scenes_cpu.py proves it on the restatements, and
tests/test_gpu_l2_scenes.py holds every device route to the normative answer, bit for bit.

The normative distance is cv::norm(a, b, NORM_L2SQR) as the reference calls it (normL2Sqr<float, double>): differences in float, squares
in double, four squares added left to right into a group, each group added to ONE running double in index order, the remainder one
element at a time, one rounding to float at the end.  l2sqr() below writes it once, with the wrong arithmetics as switches; it is NOT a
new definition: the CPU test holds it bit for bit to _refresh_ref.l2sqr, _proj_ref.l2sqr (which _bow_ref and _stereo_ref call) and
to the C oracle on every row of every scene.

How a duel is isolated inside a larger scene: the last coordinate of a row is its TAG.  The three rows of a duel carry the same tag (a
difference of exactly 0, which adds +0.0 in every arithmetic), duels differ by 2 or more in it (a distance >= 4, above every threshold
used here), and filler rows sit at tags from FILLER_TAG on.  Every duel distance is below 2.
"""
import contextlib
import importlib

import numpy as np

import _proj_ref
import _refresh_ref

f32, f64 = np.float32, np.float64

# name -> what a kernel would be doing
WRONG = {
    "f32_sum": "squares and running sum in float",
    "f32_square": "square in float, sum in double (the DBoW2 form of k_bow.hip)",
    "f64_diff": "(double)a - (double)b instead of the float difference",
    "ungrouped": "every square added to the running double on its own",
    "small_first": "the terms added in reversed order: the small ones before the large one (see the limit below)",
    "part_restart": "the running double is not carried over a 128-float part: parts summed from 0, then added",
    "tail_first": "the dim % 4 remainder added before the groups",
    "flushed_result": "a denormal float result becomes 0",
}
# The limit of small_first: it is modelled as the terms (groups of four, then the remainder) in reversed order ONLY.  A per-lane tree, two
# accumulators or a reordering inside a group are other members of that family and have no switch here.  With two terms the reversed sum
# is the normative one (addition commutes), so at 8 floats - the small dimension of the bow, projection and stereo routes - no order of
# the terms is told apart; those routes are pinned against reordering at 64 floats alone.
PART = 128          # floats per part of k_l2_topk_pairs_split
TH = 3.0            # above every duel distance, below every distance between rows of different tags
FILLER_TAG = 1000.0
TINY = np.finfo(np.float32).tiny


def _seq(t, acc):
    """t[:, 0] + t[:, 1] + ... left to right in `acc` precision (np.cumsum walks an axis sequentially; np.sum adds pairwise)"""
    if t.shape[1] == 0:
        return np.zeros(t.shape[0], acc)
    return np.cumsum(t, axis=1, dtype=acc)[:, -1]


def l2sqr(a, rows, wrong=None):
    """distance of the float row a to every row of rows -> float32 [len(rows)]; wrong: None (normative) | a key of WRONG"""
    assert wrong is None or wrong in WRONG, wrong
    a = np.asarray(a, f32)
    rows = np.asarray(rows, f32).reshape(-1, len(a))
    n, dim = rows.shape
    if n == 0:
        return np.zeros(0, f32)
    if wrong == "f64_diff":
        v = a.astype(f64)[None, :] - rows.astype(f64)
    else:
        v = a[None, :] - rows                                   # float32: one rounding
    sq = f32 if wrong in ("f32_sum", "f32_square") else f64
    acc = f32 if wrong == "f32_sum" else f64
    v = v.astype(sq)
    q = (v * v).astype(acc)                                     # one rounding in sq; exact in double (24-bit factors)
    n4 = dim // 4 * 4
    if wrong == "ungrouped":
        groups = q[:, :n4]
    else:
        g = q[:, :n4].reshape(n, -1, 4)
        groups = ((g[:, :, 0] + g[:, :, 1]) + g[:, :, 2]) + g[:, :, 3]
    tail = q[:, n4:]
    with np.errstate(under="ignore"):
        if wrong == "part_restart":
            per = PART // 4
            parts = [_seq(groups[:, k:k + per], acc) for k in range(0, groups.shape[1], per)]
            s = _seq(np.concatenate([np.stack(parts, axis=1), tail], axis=1), acc)
        else:
            terms = np.concatenate([tail, groups] if wrong == "tail_first" else [groups, tail], axis=1)
            if wrong == "small_first":
                terms = terms[:, ::-1]
            s = _seq(terms, acc)
        out = s.astype(f32)                                     # the one rounding to float
    if wrong == "flushed_result":
        out[np.abs(out) < TINY] = f32(0.0)
    return out


def l2sqr_pair(a, b, wrong=None):
    return l2sqr(a, np.asarray(b, f32)[None, :], wrong)[0]


@contextlib.contextmanager
def arithmetic(wrong):
    """inside this block the restatements evaluate float rows with `wrong`: _proj_ref (and _bow_ref / _stereo_ref / _points_ref through
    it) and _refresh_ref each read their distance from a DISTANCE dict, and this is the one place that writes to them"""
    old = _proj_ref.DISTANCE["l2sqr"], _refresh_ref.DISTANCE["l2sqr"]
    if wrong:
        _proj_ref.DISTANCE["l2sqr"] = lambda a, rows: l2sqr(a, rows, wrong)
    # distinctive() asks for the same pair of rows again and again where observations repeat (the scenes of 67 rows hold three distinct
    # ones): each pair is evaluated once per block, by the restatement's own function where no wrong arithmetic is asked for
    pair, memo = ((lambda a, b: l2sqr_pair(a, b, wrong)) if wrong else old[1]), {}

    def pair_once(a, b):
        key = (np.asarray(a).tobytes(), np.asarray(b).tobytes())
        if key not in memo:
            memo[key] = pair(a, b)
        return memo[key]
    _refresh_ref.DISTANCE["l2sqr"] = pair_once
    try:
        yield
    finally:
        _proj_ref.DISTANCE["l2sqr"], _refresh_ref.DISTANCE["l2sqr"] = old


def _afv():
    return importlib.import_module("anyfeature-vslam_amd")


def _synth():
    return _afv().synth


def _cmp(d, k):
    """three-way order of candidate k against candidate k + 1"""
    return int(d[k] > d[k + 1]) - int(d[k] < d[k + 1])


class Duel:
    """q, a, b: float32 [dim] with coordinate dim - 1 (the tag) zero in all three; how: one line on where it comes from"""

    def __init__(self, wrong, dim, q, a, b, how):
        self.wrong, self.dim, self.how = wrong, dim, how
        self.q, self.a, self.b = (np.ascontiguousarray(v, f32) for v in (q, a, b))
        assert self.q[-1] == 0 and self.a[-1] == 0 and self.b[-1] == 0
        ab = np.stack([self.a, self.b])
        self.norm, self.bad = l2sqr(self.q, ab), l2sqr(self.q, ab, wrong)
        assert _cmp(self.norm, 0) != _cmp(self.bad, 0), (wrong, dim, how, self.norm, self.bad)
        assert float(self.norm.max()) < 2.0 and float(self.bad.max()) < 2.0
        ulp = np.abs(self.norm.view(np.int32).astype(np.int64)[0] - self.norm.view(np.int32).astype(np.int64)[1])
        assert ulp <= 1 or wrong == "flushed_result", (wrong, dim, how, self.norm)

    def swapped(self):
        return Duel(self.wrong, self.dim, self.q, self.b, self.a, self.how + ", swapped")


def applies(wrong, dim):
    """can the wrong arithmetic differ from the normative one at this dimension at all"""
    if wrong == "part_restart":
        return dim > PART
    if wrong == "tail_first":
        return dim % 4 != 0 and dim > 4
    if wrong == "ungrouped":
        return dim // 4 >= 2            # the first group starts from 0: it is the same sum either way
    if wrong == "small_first":
        return dim // 4 + dim % 4 >= 3  # two terms commute
    return True


def _analytic(wrong, dim):
    """the hand-built family: the query is 0; a candidate holds 1 and 2^-12 (squares 2^24 and 1 in units of 2^-24: the float midpoint
    2^24 + 1) and small elements t elsewhere, whose squares decide on which side of the midpoint the double lands - if they survive the
    additions, which is where the orders differ.  The opponent's distance is 2^24 or 2^24 + 2 in any order.  Which member of the family
    tells `wrong` apart at `dim` is found by evaluating them all, not assumed."""
    last = dim - 1                                  # the tag: stays 0
    n4 = dim // 4 * 4
    big_at = [0]
    if n4 < last - 1:
        big_at.append(n4)                           # in the remainder
    if dim > PART + 2:
        big_at.append(PART)                         # first floats of the second part
    cands, hows = [], []
    for p0 in big_at:
        for where in ("all", "later_parts", "first_part", "tail", "groups"):
            sel = np.ones(dim, bool)
            if where == "later_parts":
                sel[:PART] = False
            elif where == "first_part":
                sel[PART:] = False
            elif where == "tail":
                sel[:n4] = False
            elif where == "groups":
                sel[n4:] = False
            sel[[p0, p0 + 1, last]] = False
            if not sel.any():
                continue
            for e in range(-34, -20):
                for m in (1.0, 1.25):
                    x = np.zeros(dim, f32)
                    x[sel] = f32(m * 2.0 ** e)
                    x[p0], x[p0 + 1] = f32(1.0), f32(2.0 ** -12)
                    cands.append(x)
                    hows.append("1, 2^-12 at %d; %g * 2^%d at %s" % (p0, m, e, where))
    opp = []
    o = np.zeros(dim, f32); o[0] = 1.0
    opp.append((o, "opponent 2^24"))
    if dim >= 4:
        o = np.zeros(dim, f32); o[0], o[1], o[2] = 1.0, 2.0 ** -12, 2.0 ** -12
        opp.append((o, "opponent 2^24 + 2"))
    X = np.stack(cands + [o for o, _ in opp])
    q = np.zeros(dim, f32)
    dn, dw = l2sqr(q, X), l2sqr(q, X, wrong)
    for k in range(len(cands)):
        for j, (o, oname) in enumerate(opp):
            jj = len(cands) + j
            pair_n, pair_w = np.array([dn[k], dn[jj]]), np.array([dw[k], dw[jj]])
            if dn[jj] != dw[jj] or _cmp(pair_n, 0) == _cmp(pair_w, 0):
                continue
            if abs(int(pair_n.view(np.int32)[0]) - int(pair_n.view(np.int32)[1])) > 1:
                continue
            return Duel(wrong, dim, q, cands[k], o, hows[k] + "; " + oname)
    return None


SEARCH_ROWS = 256
# (wrong, dim) -> (seed, row): found by find_seeds() on the CPU; only what was found is kept here
SEEDS = {
    ("f32_square", 7): (0, 18), ("f32_square", 8): (0, 1), ("f32_square", 36): (0, 48), ("f32_square", 64): (0, 69),
    ("f32_square", 100): (0, 51), ("f32_square", 128): (0, 35), ("f32_square", 200): (1, 8), ("f32_square", 256): (0, 113),
    ("f32_square", 1024): (0, 148),
    ("f64_diff", 7): (0, 0), ("f64_diff", 8): (0, 1), ("f64_diff", 36): (0, 3), ("f64_diff", 64): (0, 78), ("f64_diff", 100): (0, 24),
    ("f64_diff", 128): (0, 13), ("f64_diff", 200): (0, 13), ("f64_diff", 256): (0, 113), ("f64_diff", 1024): (1, 176),
}


def _searched_rows(dim, seed):
    """a query in [0, 1) and SEARCH_ROWS candidates of mixed magnitude (so that the float difference rounds), 24 random mantissa bits each,
    scaled so that the distances stay below 1; coordinate 0 of the query and the tag are 0"""
    s = _synth()
    scale = f32(2.0 ** -int(np.ceil(np.log2(dim) / 2)))
    st = s.lcg_states(7000 + seed, (SEARCH_ROWS + 1) * dim)
    m = ((st >> np.uint32(8)).astype(f32) * f32(2.0 ** -24)).reshape(SEARCH_ROWS + 1, dim)
    k = (s.lcg_states(9000 + seed, (SEARCH_ROWS + 1) * dim) >> np.uint32(13)) % 6
    m = m * (f32(2.0) ** (-k.astype(f32))).reshape(SEARCH_ROWS + 1, dim) * scale
    q, rows = m[0].copy(), m[1:].copy()
    q[0] = q[-1] = 0
    rows[:, -1] = 0
    return q, rows


def _single(q, target):
    """a row that differs from q in coordinate 0 alone (q[0] = 0) and whose distance is `target` in every arithmetic, or None"""
    r = np.sqrt(f64(target))
    for d in (f32(r), np.nextafter(f32(r), f32(0)), np.nextafter(f32(r), f32(4))):
        if f32(f64(d) * f64(d)) == target and f32(d * d) == target:
            b = q.copy()
            b[0] = -d
            return b
    return None


def _searched_at(wrong, dim, seed, row=None):
    q, rows = _searched_rows(dim, seed)
    dn, dw = l2sqr(q, rows), l2sqr(q, rows, wrong)
    for r in (np.flatnonzero(dn != dw) if row is None else [row]):
        if abs(int(dn.view(np.int32)[r]) - int(dw.view(np.int32)[r])) != 1:
            continue
        b = _single(q, min(dn[r], dw[r]))
        if b is None:
            continue
        both = l2sqr(q, b[None, :]), l2sqr(q, b[None, :], wrong)
        if both[0][0] != both[1][0]:
            continue
        return Duel(wrong, dim, q, rows[r], b, "searched: seed %d row %d" % (seed, r)), int(r)
    return None, -1


def find_seeds(wrongs=("f32_square", "f64_diff"), dims=(7, 8, 36, 64, 100, 128, 200, 256, 1024), nseeds=400):
    """the search whose findings SEEDS holds (run by hand when a dimension is added)"""
    out = {}
    for w in wrongs:
        for dim in dims:
            for seed in range(nseeds):
                d, r = _searched_at(w, dim, seed)
                if d is not None:
                    out[(w, dim)] = (seed, r)
                    break
            else:
                raise AssertionError("no duel found for %s at dim %d in %d seeds" % (w, dim, nseeds))
    return out


def _flushed(dim):
    q = np.zeros(dim, f32)
    a = q.copy()
    a[0] = f32(-1e-20)          # the difference is 1e-20f, the distance the denormal 1e-40f
    return Duel("flushed_result", dim, q, a, q.copy(), "one element differs by 1e-20f; the opponent is an exact duplicate")


_DUELS = {}


def duel(wrong, dim):
    """the duel of (wrong, dim), or None where the arithmetic cannot differ at this dimension (applies())"""
    key = (wrong, dim)
    if key not in _DUELS:
        d = None
        if not applies(wrong, dim):
            d = None
        elif wrong == "flushed_result":
            d = _flushed(dim)
        elif wrong in ("f32_square", "f64_diff"):
            if key not in SEEDS:
                raise AssertionError("no committed seed for %s at dim %d: run find_seeds()" % key)
            d, _ = _searched_at(wrong, dim, *SEEDS[key])
            if d is None:
                raise AssertionError("the committed seed of %s at dim %d does not give a duel" % key)
        else:
            d = _analytic(wrong, dim)
            if d is None:
                raise AssertionError("the analytic family has no duel for %s at dim %d" % key)
        _DUELS[key] = d
    return _DUELS[key]


# ================================================================ routes ================================================================
# route -> the dimensions its device test runs (tests/test_gpu_l2_scenes.py says which kernel text each one reaches)
ROUTES = {
    "match_tiled": (64, 128),                       # l2_topk_body through k_l2_topk<64|128>, k_l2_merge, k_l2_resolve
    "match_generic": (100, 7),                      # l2sqr of k_tri_row.h in the generic match_l2 kernel; 7: its remainder loop
    "match_pairs": (64, 128, 256, 36, 200, 1024),   # k_l2_topk_pairs<64|128>, k_l2_topk_pairs_split<256|0>, k_l2_resolve_pairs
    "rescan": (64, 256),                            # l2_exact in k_l2_resolve (64) and k_l2_resolve_pairs (64, 256)
    "bow": (8, 64),                                 # l2sqr of k_tri_row.h: SearchByBoW (KF, KF), (KF, F), SearchForTriangulation
    "projection": (8, 64),                          # proj_l2sqr
    "stereo": (8, 64),                              # stereo_l2sqr
    "distinctive": (36, 128, 7),                    # l2sqr of k_tri_row.h in k_match.hip's median kernels (host rows: any width, 7 reaches
                                                    # the remainder loop) and in k_refresh.hip (table rows: REFRESH_DIMS)
}
REFRESH_DIMS = (36, 128)
_NO_PARTS = "the route sums a row in one piece: there is no part boundary to restart at"
# why a route has no dim % 4 remainder: the argument check that refuses such a row, by route.  tests/test_gpu_l2_scenes.py sends each of
# these routes rows of 7 floats and sees the refusal, so a route cannot be listed here because of the dimensions it happens to be run at
REFUSES_TAIL = {
    "match_tiled": "the tiled kernels exist for 64 and 128 floats; afv_launch_match_l2_tiled returns 0 for any other dimension, which then takes the generic kernel (match_generic)",
    "match_pairs": "afv_launch_match_l2_pairs returns 0 for dim & 3 (k_match_l2.hip), afv_table_create_f32 refuses float_dim & 3 (afv_comm.hip) and afv_match_l2_pairs_device takes 64 and 128 only",
    "rescan": "l2_exact runs behind the tiled kernels (64, 128) and the table's (float_dim & 3 refused by afv_table_create_f32); the generic kernel has no rescan",
    "bow": "validate_job (afv_api.hip) refuses desc_bytes & 15, i.e. rows that are no multiple of 4 floats; table slots: afv_table_create_f32",
    "projection": "the projection jobs refuse fdim & 3 (afv_project.hip); resident frames and point stores refuse float_dim & 3 (afv_frame.hip, afv_points.hip)",
    "stereo": "a resident frame refuses float_dim & 3 at creation (afv_frame.hip)",
}
# (wrong, route) -> why no scene can exist; tests/test_l2_scenes_cpu.py checks that this is exactly the set of cells without a scene
UNREACHABLE = {
    ("part_restart", "match_tiled"): _NO_PARTS, ("part_restart", "match_generic"): _NO_PARTS, ("part_restart", "bow"): _NO_PARTS,
    ("part_restart", "projection"): _NO_PARTS, ("part_restart", "stereo"): _NO_PARTS, ("part_restart", "distinctive"): _NO_PARTS,
    ("part_restart", "rescan"): "l2_exact walks the whole row from global memory; the parts belong to the top-k kernels (match_pairs)",
    ("flushed_result", "rescan"): "the rescan needs four columns nearer than the duel pair, and nothing is nearer than a duplicate at distance 0",
}
UNREACHABLE.update({("tail_first", r): why for r, why in REFUSES_TAIL.items()})


def cells():
    """every reachable (wrong, route) with the dimensions that carry a scene"""
    out = {}
    for w in WRONG:
        for r, dims in ROUTES.items():
            if (w, r) in UNREACHABLE:
                continue
            out[(w, r)] = [d for d in dims if applies(w, d)]
    return out


def tagged(row, tag):
    r = np.array(row, f32)
    r[-1] = f32(tag)
    return r


def filler(dim, k):
    """far from every duel row and from every other filler (tags differ by 2 or more)"""
    r = np.zeros(dim, f32)
    r[0] = f32(0.25) * f32(k % 7)
    r[-1] = f32(FILLER_TAG + 2 * k)
    return r


class Scene:
    """name, wrong, route, dim, inputs (a dict of arrays), run(inputs) -> the outcome as a tuple of arrays / ints under the arithmetic that
    is installed at the time (arithmetic() above)"""

    def __init__(self, route, d, what, inputs, run):
        self.route, self.wrong, self.dim, self.duel = route, d.wrong, d.dim, d
        self.name = "%s-%s-%d-%s" % (route, d.wrong, d.dim, what)
        self.inputs, self._run = inputs, run
        self._outcome = {}

    def outcome(self, wrong=None):
        if wrong not in self._outcome:
            with arithmetic(wrong):
                self._outcome[wrong] = self._run(self.inputs)
        return self._outcome[wrong]

    @property
    def expected(self):
        return self.outcome(None)

    def flips(self):
        return not same(self.expected, self.outcome(self.wrong))


def same(a, b):
    return len(a) == len(b) and all(np.asarray(x).dtype == np.asarray(y).dtype and np.asarray(x).tobytes() == np.asarray(y).tobytes()
                                    for x, y in zip(a, b))


def _oriented(make, d):
    """the scene of duel d, with A and B in the order in which its outcome depends on the arithmetic (first-of-equals and last-of-equals
    routes want opposite orders); found by running the restatement, as _quant_scenes._order_scene finds its seeds"""
    for dd in (d, d.swapped()):
        s = make(dd)
        if s.flips():
            return s
    raise AssertionError("no order of the duel %s at dim %d changes the outcome of %s" % (d.wrong, d.dim, s.name))


# ---- the greedy brute-force matcher (match_l2, match_l2_pairs_device, DescriptorTable.match_pairs) ----
N1, N2 = 65, 67     # two row tiles; three 32-column chunks (nine 8-column chunks at 1024 floats)
NDUEL = 33


def _run_greedy(inp):
    import _bow_ref
    out, nm, _ = _bow_ref.search_by_bow_kf_kf(inp["d1"], inp["d2"], valid1=inp.get("valid1"), valid2=inp.get("valid2"), th_low=TH, nnratio=1.0)
    return out, np.int32(nm)


def match_scene(route, d, masks=False):
    """33 duel queries: duel t < 32 sits in row 2 t (the even lanes of BOTH halves of the first row tile's wavefront, so the partial sums
    parked for lanes 32 .. 63 decide matches too), duel 32 in row 64 (the second row tile).  Duel t < 32 has its candidates at the columns
    t (first chunk, every position 0 .. 31 of a staged chunk, 0 .. 7 of the narrow one) and 33 + t (a later chunk, every position again);
    duel 32 at 32 and 65.  Odd duels hold A and B exchanged.  nnratio = 1: equal distances give no match, unequal ones the nearer column."""
    dim = d.dim
    d1 = np.stack([filler(dim, k) for k in range(N1)])
    d2 = np.stack([filler(dim, 500 + k) for k in range(N2)])
    sw = d.swapped()
    for t in range(NDUEL):
        r = 2 * t
        dd = sw if t % 2 else d
        ca, cb = (t, 33 + t) if t < 32 else (32, 65)
        d1[r], d2[ca], d2[cb] = tagged(dd.q, 2 * t), tagged(dd.a, 2 * t), tagged(dd.b, 2 * t)
    inp = {"d1": d1, "d2": d2}
    if masks:
        v1, v2 = np.ones(N1, np.uint8), np.ones(N2, np.uint8)
        v1[[6, 41, 64]] = 0             # a duel row, a filler row, the row of the second tile
        v2[[5, 66, 33 + 8]] = 0         # the first candidate of duel 5, a filler column, the second candidate of duel 8
        inp.update(valid1=v1, valid2=v2)
    return Scene(route, d, "masks" if masks else "plain", inp, _run_greedy)


def rescan_scene(d):
    """rows 0 .. 3 equal columns 0 .. 3 and take them; row 4, the duel query, has those four columns as its nearest, so its key list is
    used up and l2_exact decides between its duel pair at the columns 5 and 7"""
    dim = d.dim
    lo = float(min(d.norm.min(), d.bad.min()))
    q = tagged(d.q, 0)
    E = []
    for k in range(4):
        e = q.copy()
        e[1 + k] += f32(np.sqrt(lo) * (k + 1) / 8.0)
        E.append(e)
    d1 = np.stack(E + [q] + [filler(dim, k) for k in range(3)])
    d2 = np.stack(E + [filler(dim, 500), tagged(d.a, 0), filler(dim, 501), tagged(d.b, 0)] + [filler(dim, 502 + k) for k in range(4)])
    for w in (None, d.wrong):
        assert set(np.argsort(l2sqr(q, d2, w), kind="stable")[:4]) == {0, 1, 2, 3}
    return Scene("rescan", d, "claimed", {"d1": d1, "d2": d2}, _run_greedy)


# ---- ComputeDistinctiveDescriptors / afv_table_refresh_points ----
def _run_distinctive(inp):
    bi, bm = _refresh_ref.distinctive(list(inp["rows"]), True, 4 * inp["rows"].shape[1])
    return np.int32(bi), f32(bm)


def distinctive_scene(d, n):
    """the observations are the duel's A, its B - or the mirror image of B about the query (the same distance to the query), whichever is
    farther from A, so that the medians are the duel's distances - and the query; n = 5 adds two far rows; n > 64 repeats the three rows
    (the medians stay the duel's distances) - the path that does not stage the N x N distances in LDS"""
    bm = (f32(2.0) * d.q - d.b).astype(f32)
    assert l2sqr_pair(d.q, bm) == d.norm[1] and l2sqr_pair(d.q, bm, d.wrong) == d.bad[1], "the mirror image keeps the distance"
    if l2sqr_pair(d.a, d.b) > l2sqr_pair(d.a, bm):
        bm = d.b
    base = [d.a, bm, d.q]
    if n <= 5:
        rows = base + [filler(d.dim, k) for k in range(n - 3)]
    else:
        rows = [base[k % 3] for k in range(n)]
    return Scene("distinctive", d, "n%d" % n, {"rows": np.stack(rows)}, _run_distinctive)


# ---- BoW-guided matchers and SearchForTriangulation ----
def bow_scenes(d):
    """one Case of tests/_match_scenes.py per kind and node shape: the duel alone ('single': one node), among 6 and among 76 filler features
    per side in several nodes"""
    import _match_scenes as MS
    out = []
    for kind in ("kfkf", "kff", "tri"):
        for shape in MS.SHAPES:
            def make(dd, kind=kind, shape=shape):
                desc = "f%d" % dd.dim
                spec = dict(rows=[{"row": dd.q}], cols=[{"row": dd.a}, {"row": dd.b}], kw={})   # (KF, F): the keyframe's row searches the frame's
                K1, K2 = MS.build(desc, spec, shape)
                kw = dict(th_low=TH)
                if kind == "tri":
                    kw.update(F12=MS.F_HLINE, epipole=MS.FAR_EPIPOLE)
                else:
                    kw.update(nnratio=1.0, check_orientation=False)
                case = MS.Case("l2-%s-%s-%s-%s" % (dd.wrong, desc, kind, shape), kind, K1, K2, kw, None)
                return Scene("bow", dd, "%s-%s" % (kind, shape), {"case": case}, lambda inp: tuple(MS.run_ref(inp["case"])[:2]))
            out.append(_oriented(make, d))
    return out


# ---- projection searches ----
PROJ_KINDS = {"localmap": dict(th_high=TH, nnratio=1.0, last_frame=False), "lastframe": dict(th_high=TH, nnratio=1.0, last_frame=True),
              "fuse": dict(th_high=TH, fuse=True), "init": dict(th_low=TH, nnratio=1.0, check_orientation=False)}
NQ = 5


def _run_proj(inp):
    c = inp["case"]
    f = _proj_ref.match_initialization if c.kind == "init" else _proj_ref.match_projection
    got, n, _ = f(c.F, c.Q, **c.kw)
    return got, np.int32(n)


def proj_scenes(d):
    """five queries 60 px apart, each with the duel pair in its own grid cell (index order = visiting order) and two far features in its
    window; one Case of tests/_proj_scenes.py per search kind"""
    import _proj_scenes as PS
    afv = PS.afv
    out = []
    for kind, kw in PROJ_KINDS.items():
        def make(dd, kind=kind, kw=kw):
            D, pts, QD, u, v = [], [], [], [], []
            for k in range(NQ):
                x0, y0 = 100.0 + 60.0 * k, 100.0
                QD.append(tagged(dd.q, 2 * k)); u.append(x0); v.append(y0)
                for row, dx in ((filler(dd.dim, 2 * k), 0.5), (tagged(dd.a, 2 * k), 1.0), (tagged(dd.b, 2 * k), 2.0), (filler(dd.dim, 2 * k + 1), 3.0)):
                    D.append(row); pts.append((x0 + dx, y0 + 1.0))
            n = len(D)
            F = afv.FrameGridView(np.stack(D), np.array(pts, f32), np.ones(n, f32), angles=np.zeros(n, f32), **PS.GRIDS["default"])
            Q = afv.ProjectionQueries(np.stack(QD), np.array(u, f32), np.array(v, f32), np.full(NQ, 5.0, f32), np.full(NQ, 0.5, f32),
                                      np.full(NQ, 2.0, f32), angles=np.zeros(NQ, f32))
            case = PS.Case("l2-%s-f%d-%s" % (dd.wrong, dd.dim, kind), "init" if kind == "init" else "proj", F, Q, dict(kw), None)
            return Scene("projection", dd, kind, {"case": case}, _run_proj)
        out.append(_oriented(make, d))
        # (Fuse answers every query on its own: nothing is taken, no key list runs out; and nothing is nearer than the duplicate at
        # distance 0 of the flushed_result duel, as in the rescan of the brute-force matcher)
        if kind != "fuse" and d.wrong != "flushed_result":
            out.append(_oriented(lambda dd, kind=kind, kw=kw: _proj_used_up(dd, kind, kw), d))
    return out


def _proj_used_up(dd, kind, kw):
    """eight queries equal eight features and take them; the ninth, the duel query, has those eight as its nearest, so the keys phase 1
    kept for it (4; 8 in SearchForInitialization) are used up and the ordered phase evaluates its window again: the rescans of
    proj_resolve, proj_resolve_wg and init_resolve"""
    import _proj_scenes as PS
    afv = PS.afv
    lo = float(min(dd.norm.min(), dd.bad.min()))
    q = tagged(dd.q, 0)
    E = []
    for k in range(8):
        e = q.copy()
        e[k % (dd.dim - 1)] += f32(np.sqrt(lo) * (k + 1) / 16.0)
        E.append(e)
    D = E + [filler(dd.dim, 0), tagged(dd.a, 0), tagged(dd.b, 0), filler(dd.dim, 1)]
    for w in (None, dd.wrong):
        assert set(np.argsort(l2sqr(q, np.stack(D), w), kind="stable")[:8]) == set(range(8))
    n = len(D)
    pts = np.array([(100.5 + 0.25 * i, 101.0) for i in range(n)], f32)
    F = afv.FrameGridView(np.stack(D), pts, np.ones(n, f32), angles=np.zeros(n, f32), **PS.GRIDS["default"])
    nq = 9
    Q = afv.ProjectionQueries(np.stack(E + [q]), np.full(nq, 100.0, f32), np.full(nq, 100.0, f32), np.full(nq, 5.0, f32), np.full(nq, 0.5, f32),
                              np.full(nq, 2.0, f32), angles=np.zeros(nq, f32))
    case = PS.Case("l2-%s-f%d-%s-used-up" % (dd.wrong, dd.dim, kind), "init" if kind == "init" else "proj", F, Q, dict(kw), None)
    return Scene("projection", dd, kind + "-used-up", {"case": case}, _run_proj)


def _run_points(inp):
    import _points_scenes as PSC
    got, n, o = PSC.expected_search(_afv(), _proj_ref, inp["scene"])
    return got, np.int32(n), np.asarray(o["in_view"], bool)


def points_scene(d):
    """SearchLocalPoints (afv_frame_search_points) over a float point store: five map points in front of the 96 x 64 camera of
    tests/_points_scenes.py, each with the duel pair and two far features next to its projection; the store holds the queries' rows"""
    import _points_ref as PR
    import _points_scenes as PSC

    def make(dd):
        n = NQ
        P = PR.Points(16, 4 * dd.dim, dd.dim)
        ids = np.arange(n)
        pos = np.array([(-2.0 + k, 0.5 * (k % 2), 4.0) for k in range(n)], f32)
        P.set(ids, pos=pos, normal=np.tile(f32([0, 0, 1]), (n, 1)), min_distance=np.full(n, 0.5, f32), max_distance=np.full(n, 100.0, f32),
              ref_size=np.ones(n, f32), ref_distance=np.full(n, 4.0, f32), ref_sigma=np.full(n, 0.5, f32))
        P.set_flags(ids, bad=np.zeros(n), observed=np.ones(n))
        P.set_descriptors(ids, np.stack([tagged(dd.q, 2 * k) for k in range(n)]))
        sc = PSC.Scene("l2-%s-f%d-points" % (dd.wrong, dd.dim), None, PR.FRUSTUM, P, PR.Camera(), ids, lambda tr: True, radius_th=2.0, th=TH,
                       nnratio=1.0)
        o = sc.project()
        assert o["in_view"].all()
        x, y, sz, rows = [], [], [], []
        for k in range(n):
            for row, dx in ((filler(dd.dim, 2 * k), -0.25), (tagged(dd.a, 2 * k), 0.25), (tagged(dd.b, 2 * k), 0.5), (filler(dd.dim, 2 * k + 1), 0.75)):
                x.append(f32(o["u"][k] + f32(dx))); y.append(o["v"][k]); sz.append(o["size"][k]); rows.append(row)
        sc.feat = PSC.Features(x, y, sz, np.stack(rows))
        return Scene("projection", dd, "points", {"scene": sc}, _run_points)
    return _oriented(make, d)


# ---- stereo ----
def stereo_scene(d):
    """one image row: a left keypoint with the duel query and two right keypoints inside its disparity window with A and B"""
    import _stereo_scenes as SS

    def make(dd):
        b = SS.Builder(41, float_dim=dd.dim)
        b.ballast()
        b.left(50, 30, desc=dd.q.copy())
        b.right(44, 30, desc=dd.a.copy())
        b.right(46, 30, desc=dd.b.copy())
        sc = b.scene("l2-%s-f%d" % (dd.wrong, dd.dim), th_high=TH, th_low=TH)
        return Scene("stereo", dd, "row", {"scene": sc}, lambda inp: tuple(inp["scene"].run()[:4]))
    return _oriented(make, d)


_SCENES = {}


def scenes(route):
    """every scene of a route, over its reachable wrong arithmetics and dimensions"""
    if route not in _SCENES:
        out = []
        for (w, r), dims in cells().items():
            if r != route:
                continue
            for dim in dims:
                d = duel(w, dim)
                if route == "match_tiled":
                    out += [match_scene(route, d), match_scene(route, d, masks=True)]
                elif route in ("match_generic", "match_pairs"):
                    out.append(match_scene(route, d))
                elif route == "rescan":
                    out.append(rescan_scene(d))
                elif route == "distinctive":
                    out += [_oriented(lambda dd, n=n: distinctive_scene(dd, n), d) for n in {36: (3, 5, 67), 7: (3, 67)}.get(dim, (3, 4))]
                elif route == "bow":
                    out += bow_scenes(d)
                elif route == "projection":
                    out += proj_scenes(d) + [points_scene(d)]
                elif route == "stereo":
                    out.append(stereo_scene(d))
        _SCENES[route] = out
    return _SCENES[route]
