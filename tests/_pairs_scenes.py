"""constructed scenes for the two-phase brute-force pair matcher: key records and contention (test data; deterministic, no GPU)

A Scene is one pair of descriptor sets (D1 rows, D2 columns) with its ratio, its orientation switch and what it exists for:
  rule / row     the class of tests/_pairs_ref.py's resolve_model (CLASSES) the named row must reach, under the record models in `models`
  flips          the keys of _pairs_ref.FLIPS the scene sits on: a record flip must break record_contract at the named row, an outcome
                 flip must change the scene's answer, a trace flip must change the class of the named row
  expect         nk / head (the first slots of the record) per record model at the named row, `tail`: a real key behind the exact prefix,
                 `cols`: the answer of single rows, `rescans`: how many rows need the exact rescan at least
tests/test_pairs_ref_cpu.py proves all of it on the CPU; tests/test_gpu_pairs_scenes.py runs the scenes through every route.

Descriptors are built from DISTANCES with base_row / row_at of _proj_scenes.py.  The row under study is the base row B, its columns are
C(d, v) = row_at(kind, d, v): d bits flipped from bit 37 v on.  A TAKER is an earlier row that is a byte copy of one column: it reaches
that column at distance 0 and takes it.  Columns that are not named are filler, rows given as an int are filler rows: further than th + 5
from everything (asserted when the scene is built).  anchor(k) is a random row far from the base and from the filler: a second place to
build around (near(row, d, v) flips d bits of any row).

Column indices matter to the matrix-core engine: column c belongs to lane half (c % 8) // 4, a tile is 64 columns, and at cap = 320 the
small-batch path deals the tiles to three slices (ceil(ntiles / 3) each).  Named columns sit in half 0 (indices 0..3, 8..11, ...) unless a
scene is about the halves, so that the exact prefix is the same four keys under every record model.

All scenes of a kind use cap = 320 and live in ONE table (table_of), set 2 i = the rows and 2 i + 1 = the columns of scene i; a call takes
one ratio, so a route is one call per RATIO GROUP (0.6 with the orientation check - the angles are 0 outside the rotation scenes, so one
bin holds every match -, 0.9 and 1.5 without).  The two large scenes (cap 1300 and cap 4096, the largest afv_match_bruteforce_pairs_device
accepts) have a table of their own.
"""
import collections

import numpy as np

import _match_scenes as MS
import _pairs_ref as P
from _proj_scenes import S, base_row, row_at

f32 = np.float32
KINDS = ("b32", "b61")
TH = {"b32": 75.0, "b61": 128.0}   # 61-byte rows: what _th(61) of tests/test_gpu_table_widths.py gives
MAXD = {"b32": 256, "b61": 488}
CAP = 320
Scene = collections.namedtuple("Scene", "name kind D1 D2 a1 a2 ratio ori cap rule row flips models expect")


def nbytes(kind):
    return int(kind[1:])


def C(kind, d, v):
    return row_at(kind, d, v)


def near(kind, row, d, v):
    return row ^ (row_at(kind, d, v) ^ base_row(kind))


def anchor(kind, k):
    return base_row(kind) ^ S.lcg_bytes(7000 + k, nbytes(kind))


def h0(i):
    """index of the i-th column of lane half 0"""
    return 8 * (i // 4) + i % 4


def _far(kind, rows, is_fill_row, cols, is_fill_col, name):
    th = TH[kind]
    dist = P.hamming(rows, cols)
    if is_fill_row.any() and dist.shape[1]:
        assert dist[is_fill_row].min() > th + 5, (name, "a filler row is near a column")
    if is_fill_col.any() and dist.shape[0]:
        assert dist[:, is_fill_col].min() > th + 5, (name, "a filler column is near a row")


def scene(kind, name, rows, cols, n2=None, ratio=0.6, ori=None, rule=None, row=None, flips=(), models=P.MODELS, expect=None, a1=None, a2=None,
          cap=CAP):
    """rows: descriptors, an int k = filler row k.  cols: {index: descriptor} (the other indices below n2 are filler) or a list"""
    B = base_row(kind)
    fill_row = np.array([isinstance(r, (int, np.integer)) for r in rows], bool)
    D1 = np.stack([MS.filler(kind, r, 0) if f else np.asarray(r, np.uint8) for r, f in zip(rows, fill_row)]) if len(rows) else np.zeros((0, len(B)), np.uint8)
    if not isinstance(cols, dict):
        cols = dict(enumerate(cols))
    n2 = (max(cols) + 1 if cols else 0) if n2 is None else n2
    assert all(0 <= c < n2 for c in cols)
    fill_col = np.array([c not in cols for c in range(n2)], bool)
    D2 = np.stack([cols[c] if c in cols else MS.filler(kind, c, 1) for c in range(n2)]) if n2 else np.zeros((0, len(B)), np.uint8)
    assert len(D1) <= cap and n2 <= cap, name
    _far(kind, D1, fill_row, D2, fill_col, name)
    ori = (ratio == 0.6) if ori is None else ori
    a1 = np.zeros(len(D1), np.float32) if a1 is None else np.asarray(a1, np.float32)
    a2 = np.zeros(n2, np.float32) if a2 is None else np.asarray(a2, np.float32)
    return Scene("%s-%s" % (name, kind), kind, np.ascontiguousarray(D1), np.ascontiguousarray(D2), a1, a2, ratio, ori, cap, rule, row, tuple(flips),
                 tuple(models), expect or {})


def key(d, c):
    return P.key_of(d, c)


# ---- decision scenes ----
def decision_scenes(kind):
    th = int(TH[kind])
    B = base_row(kind)
    c = lambda d, v: C(kind, d, v)
    out = []
    add = lambda *a, **k: out.append(scene(kind, *a, **k))
    add("keys_accept", [B], {0: c(10, 1), 1: c(40, 2)}, n2=24, rule="keys_accept", row=0, expect=dict(cols={0: 0}))
    # 0.6f * 50.0f = 30.000002: a best distance of 30 is accepted, although 0.6 * 50 is 30 (_bow_ref.FLIPS["ratio_f32"])
    assert f32(0.6) * f32(50) > f32(30) and not 30.0 < 0.6 * 50.0
    add("ratio_f32_accepts_30", [B], {0: c(30, 1), 1: c(50, 2)}, n2=24, rule="keys_accept", row=0, expect=dict(cols={0: 0}))
    assert f32(0.9) * f32(10) == f32(9)
    add("keys_reject_ratio_eq", [B], {0: c(9, 1), 1: c(10, 2)}, n2=24, ratio=0.9, rule="keys_reject", row=0, expect=dict(cols={0: -1}))
    k = {0: c(10, 1), 1: c(th, 2)}
    add("best_fails_th_at_th", [k[0], B], k, n2=24, rule="best_fails_th", row=1, expect=dict(cols={0: 0, 1: -1}))
    k = {0: c(5, 1), 1: c(30, 2)}
    add("dead_between_live", [0, B, 1, 2, B], k, n2=24, rule="dead", row=2, flips=("dead_kept_live",), expect=dict(cols={1: 0, 4: 1}, slots={1: 0, 4: 1}))
    # three takers in front; the key that is left is the row's FIRST, not its last exact one; the true next column is filler
    k = {0: c(10, 1), 1: c(30, 2), 2: c(31, 3), 3: c(32, 4)}
    add("bound_accept", [k[1], k[2], k[3], B], k, n2=24, rule="bound_accept", row=3, expect=dict(cols={3: 0}))
    # ... at equality: 9 < 0.9f * 10 fails, the rescan finds the fifth column AT last_d = 10 and refuses; <= would have accepted
    k = {0: c(9, 1), 1: c(10, 2), 2: c(10, 3), 3: c(10, 4), 8: c(10, 5)}
    add("bound_eq_column_at_last_d", [k[1], k[2], k[3], B], k, n2=24, ratio=0.9, rule="rescan_none", row=3, flips=("bound_le",), expect=dict(cols={3: -1}))
    # the rescan of row 3 takes X = column 0, which row 4 (a byte copy of X, later in the same round) had claimed
    k = {0: c(30, 1), 1: c(31, 2), 2: c(32, 3), 3: c(33, 4)}
    add("rescan_take_claimed_behind", [k[1], k[2], k[3], B, k[0]], k, n2=24, rule="rescan_take", row=3, flips=("rescan_sees_taken",),
        expect=dict(cols={3: 0, 4: -1}))
    # the seven nearest are taken (every exact key, whatever nk): the rescan takes the 8th nearest / finds two close ones and refuses
    k = {i: c(10 + i, 1 + i) for i in range(7)}
    k[7] = c(20, 9)
    add("rescan_beyond_keys_takes_8th", [k[i] for i in range(7)] + [B], k, n2=24, rule="rescan_take", row=7, expect=dict(cols={7: 7}))
    k = dict(k)
    k[12] = c(22, 10)
    add("rescan_beyond_keys_refuses", [k[i] for i in range(7)] + [B], k, n2=24, rule="rescan_none", row=7, expect=dict(cols={7: -1}))
    k = {0: c(10, 1), 1: c(20, 2), 2: c(30, 3), 3: c(th, 4)}
    add("nokey_bound_fail", [k[0], k[1], k[2], k[3], B], k, n2=24, rule="nokey_bound_fail", row=4, flips=("nokey_le",), expect=dict(cols={4: -1}))
    for n in (1, 2, 3):   # the whole list is there and taken: a NO_KEY inside the exact prefix
        k = {i: c(10 + 5 * i, 1 + i) for i in range(n)}
        add("complete_n%d_all_taken" % n, [k[i] for i in range(n)] + [B], k, n2=n, rule="complete_list", row=n,
            flips=("complete_ignored",) if n == 2 else (), expect=dict(cols={n: -1}))
    # four columns, four exact keys, no NO_KEY in the prefix: only n2 > nk says that the list is complete
    k = {i: c(10 + 5 * i, 1 + i) for i in range(4)}
    add("complete_n4_guard_all_taken", [k[0], k[1], k[2], k[3], B], k, n2=4, rule="complete_list", row=4, flips=("guard_dropped",), expect=dict(cols={4: -1}))
    add("complete_n4_guard_one_left", [k[1], k[2], k[3], B], k, n2=4, rule="complete_list", row=3, flips=("guard_dropped",), expect=dict(cols={3: 0}))
    # rescans whose best free column lies behind index 256 and at n2 - 1: the strided scan loops and their clamped last loads
    k = {0: c(5, 1), 1: c(6, 2), 2: c(7, 3), 3: c(8, 4), 260: c(12, 5), 299: c(25, 6)}
    add("rescan_far_index", [k[0], k[1], k[2], k[3], B, B], k, n2=300, rule="rescan_take", row=5, expect=dict(cols={4: 260, 5: 299}))
    k = {0: c(5, 1), 1: c(6, 2), 2: c(7, 3), 3: c(8, 4), 9: c(20, 5), 17: c(40, 6), 30: c(40, 7)}
    add("rescan_equal_seconds", [k[0], k[1], k[2], k[3], B], k, n2=40, rule="rescan_take", row=4, expect=dict(cols={4: 9}))
    k = {0: c(5, 1), 1: c(6, 2), 2: c(7, 3), 3: c(8, 4), 9: c(20, 5), 17: c(20, 6)}
    add("rescan_tie_lower_column", [k[0], k[1], k[2], k[3], B], k, n2=40, ratio=1.5, rule="rescan_take", row=4, flips=("rescan_tie_high",), expect=dict(cols={4: 9}))
    return out


def chain_scenes(kind):
    """row i sees columns i - 1 and i at distance 1 and every other column at 3; row 0 IS column 0 (_match_scenes.chain): every row loses
    its first choice to the row before it, all the way down"""
    B = base_row(kind)
    out = []
    for n in (2, 5, 64, 65, 130):
        cols = [MS.distinct(kind, i) for i in range(n)]
        rows = [cols[0]] + [cols[i] ^ cols[i - 1] ^ B for i in range(1, n)]
        out.append(scene(kind, "chain_%d" % n, rows, cols, expect=dict(cols={i: i for i in range(n)})))
    return out


def wg_list_scenes(kind):
    """the waiting list of the workgroup form: rows that need the exact rescan after one convergence.  K0..K3 near the base are taken, so
    every copy of B waits; its rescan finds 20 and 22 and refuses.  Z = anchor(1) has its own four taken neighbours Y0..Y3 and a free
    column X: a waiting row whose rescan TAKES"""
    B, Z = base_row(kind), anchor(kind, 1)
    c = lambda d, v: C(kind, d, v)
    k = {0: c(5, 1), 1: c(6, 2), 2: c(7, 3), 3: c(8, 4), 9: c(20, 5), 17: c(22, 6)}
    out = [scene(kind, "wg_33_waiting_none_takes", [k[0], k[1], k[2], k[3]] + [B] * 33, k, n2=24, rule="rescan_none", row=36, expect=dict(rescans=33))]
    kz = dict(k)
    for i in range(4):
        kz[32 + i] = near(kind, Z, 1 + i, 20 + i)
    kz[40] = near(kind, Z, 6, 30)
    takers = [kz[i] for i in (0, 1, 2, 3, 32, 33, 34, 35)]
    out.append(scene(kind, "wg_40_waiting_17th_takes", takers + [B] * 16 + [Z] + [B] * 23, kz, n2=48, rule="rescan_take", row=24,
                     expect=dict(rescans=40, cols={23: -1, 24: 40, 25: -1})))
    out.append(scene(kind, "wg_130_waiting_last_takes", takers + [B] * 129 + [Z], kz, n2=48, rule="rescan_take", row=137,
                     expect=dict(rescans=130, cols={136: -1, 137: 40})))
    return out


def rotation_scenes(kind):
    """three generators of _match_scenes.py: both resolve kernels carry their own copy of the histogram"""
    by = {c.name: c for c in MS.rotation_scenes(kind)}
    out = []
    for name in ("rot_wrap", "max_first", "max2_lt-100"):
        c = by["%s-%s-kfkf-single" % (name, kind)]
        assert c.kw["check_orientation"] and c.kw["nnratio"] == 0.6 and c.K1.featvec is None
        out.append(scene(kind, name.replace("-", "_"), list(c.K1.descriptors), list(c.K2.descriptors), a1=c.K1.angles, a2=c.K2.angles, ori=True))
    return out


# ---- record scenes ----
N2S = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 257)
N1S = (1, 63, 64, 65, 255, 256, 257)


def record_scenes(kind):
    th = int(TH[kind])
    B = base_row(kind)
    c = lambda d, v: C(kind, d, v)
    out = []
    add = lambda *a, **k: out.append(scene(kind, *a, **k))
    # sizes on the edges of the halves (4, 8), the tiles (64) and the row tiles (256), paired one to one; near rows and columns: ties, contention
    for j, n2 in enumerate(N2S):
        n1 = N1S[j % len(N1S)]
        add("sizes_%dx%d" % (n1, n2), [c(i % 7, 200 + i) for i in range(n1)], [c(2 + (q * 11) % 67, q) for q in range(n2)], ratio=0.9)
    # the four nearest over the lane halves (columns 0..3 = half 0, 4..7 = half 1): each exact-prefix length the merge can give
    halves = {
        "nk4_split_4_0": ([5, 6, 7, 8, 30, 31, 32, 33], 4),    # t = the 4th key of half 0 = the row's 4th nearest
        "nk5_split_3_1": ([5, 6, 7, 40, 8, 50, 51, 52], 5),    # half 0's fourth (40) bounds: 5 6 7 8 40 | 50 51
        "nk6_split_2_2": ([5, 6, 40, 41, 7, 8, 50, 51], 6),    # half 0's fourth (41) bounds: 5 6 7 8 40 41 | 50
        "nk7_split_3_1": ([5, 6, 7, 60, 8, 20, 21, 22], 7),    # half 1's fourth (22) bounds and is the seventh key
    }
    for name, (ds, nk) in halves.items():
        head = sorted(key(d, q) for q, d in enumerate(ds))[:7]
        add(name, [B], {q: c(d, 1 + q) for q, d in enumerate(ds)}, n2=24, row=0,
            expect=dict(nk={"popcount": 4, "mfma": nk, "sliced": nk}, head={"popcount": head[:4], "mfma": head, "sliced": head}))
    # equal distances across the halves (3 | 4), a tile boundary (63 | 64) and a slice boundary (127 | 128 at cap 320): the lower column first
    k = {3: c(10, 1), 4: c(10, 2), 63: c(11, 3), 64: c(11, 4), 127: c(12, 5), 128: c(12, 6)}
    head = [key(10, 3), key(10, 4), key(11, 63), key(11, 64), key(12, 127), key(12, 128)]
    add("ties_across_half_tile_slice", [B], k, n2=257, row=0, expect=dict(head={"popcount": head[:4], "mfma": head, "sliced": head}))
    # the single nearest column is the LAST of a set with n2 % 64 == 1: the clamped rows of the partial tile are copies of it
    for n2 in (65, 257):
        add("nearest_is_last_column_%d" % n2, [B], {n2 - 1: c(5, 1)}, n2=n2, row=0, rule="keys_accept", expect=dict(head={m: [key(5, n2 - 1)] for m in P.MODELS}, second_far=True))
    A = [anchor(kind, 2 + i) for i in range(3)]
    k = {63: near(kind, A[0], 5, 1), 64: near(kind, A[1], 5, 2), 199: near(kind, A[2], 5, 3)}
    add("nearest_at_63_64_last", A, k, n2=200, expect=dict(cols={0: 63, 1: 64, 2: 199}))
    # distance 0 and the largest distance of the kind: an all-zero row against an all-one column and the reverse
    z, o = np.zeros(nbytes(kind), np.uint8), np.full(nbytes(kind), 255, np.uint8)
    add("distance_0_and_max", [z, o], [o, z], row=0, expect=dict(head={m: [key(0, 1), key(MAXD[kind], 0)] for m in P.MODELS}, cols={0: 1, 1: 0}))
    # the 5th..7th slots hold real keys that are NOT the next nearest (column 8 at 10 is hidden behind half 0's four); the four nearest are
    # taken, the rescan takes column 8; a prefix read one key too long decides on 40 against 41 and refuses
    k = {0: c(1, 1), 1: c(2, 2), 2: c(3, 3), 3: c(4, 4), 4: c(40, 5), 5: c(41, 6), 6: c(42, 7), 7: c(43, 8), 8: c(10, 9)}
    head = [key(1, 0), key(2, 1), key(3, 2), key(4, 3), key(40, 4), key(41, 5), key(42, 6)]
    exp = dict(nk={m: 4 for m in P.MODELS}, head={"popcount": head[:4], "mfma": head, "sliced": head}, tail=("mfma", "sliced"), cols={4: 8})
    add("tail_not_nearest", [k[0], k[1], k[2], k[3], B], k, n2=24, rule="rescan_take", row=4, flips=("nk_plus1", "tail_exact"), expect=exp)
    # the same over three slices (columns 0..127 | 128..255 | 256): the merged record holds slice 0's inexact tail ABOVE the bound
    add("sliced_tail_above_bound", [k[0], k[1], k[2], k[3], B], k, n2=257, rule="rescan_take", row=4, flips=("slice_bound", "nk_plus1", "tail_exact"), expect=exp)
    # all seven nearest in one slice (the middle one) / dealt over the three slices of cap 320 (one per slice needs seven slices: that
    # row lives in the cap 1300 scene)
    k = {128 + q: c(5 + q, 1 + q) for q in range(7)}
    head = [key(5 + q, 128 + q) for q in range(7)]
    add("seven_in_one_slice", [B], k, n2=257, row=0, expect=dict(head={"popcount": head[:4], "mfma": head, "sliced": head}))
    idx = (0, 128, 256, 1, 132, 5, 133)
    k = {q: c(5 + i, 1 + i) for i, q in enumerate(idx)}
    head = [key(5 + i, q) for i, q in enumerate(idx)]
    add("seven_over_three_slices", [B], k, n2=257, row=0, expect=dict(head={"popcount": head[:4], "mfma": head, "sliced": head}))
    # a set so small that two of the three slices have no tile: any n2 <= 64 (sizes_1x1 ... ); named here for the per-slice check
    add("most_slices_empty", [B, B], {0: c(5, 1), 1: c(30, 2)}, n2=2, row=0, expect=dict(empty_slices=(1, 2), cols={0: 0, 1: 1}))
    return out


def small_scenes(kind):
    out = decision_scenes(kind) + chain_scenes(kind) + wg_list_scenes(kind) + rotation_scenes(kind) + record_scenes(kind)
    assert len({s.name for s in out}) == len(out)
    return out


# ---- the two large scenes ----
def _random_rows(kind, seed, n):
    """independent random rows (a RandomState of their own, no global state).  Not the LCG of afv.synth: a thousand of its 32-byte rows hold
    pairs only 32 bits apart, and these rows must be far from each other"""
    return np.random.RandomState(seed).randint(0, 256, (n, nbytes(kind))).astype(np.uint8)


def live_behind_1024(kind, n=1100, cap=1300):
    """row i IS column i for 1100 random rows: about 1090 live rows without contention (a row whose column was given away is dead when
    nothing else is nearer than th: at most 13 of them, all 61-byte ones, so row 1032 is live slot 1025 at the least).  Behind live slot
    1024: takers of columns 1040..1043 (rows 1032..1035), and two copies of B (rows 1036, 1037) whose four exact keys are those
    columns: both need the exact rescan, the first takes column 1044 (20 against 40), the second column 1045 (40 against filler).  Their
    records are read from global memory (PAIR_KEYS_LDS = 1024) and the workgroup form finds them on its one-at-a-time path.
    Row 5 is anchor(9); its seven nearest columns lie ONE PER SLICE (11 slices at cap 1300, two tiles = 128 columns each)"""
    B = base_row(kind)
    D = _random_rows(kind, 50000 + nbytes(kind), n)
    D1, D2 = D.copy(), D.copy()
    for i, d in enumerate((5, 6, 7, 8)):
        D2[1040 + i] = C(kind, d, 1 + i)
        D1[1032 + i] = D2[1040 + i]
    D2[1044], D2[1045] = C(kind, 20, 5), C(kind, 40, 6)
    D1[1036] = D1[1037] = B
    Z = anchor(kind, 9)
    D1[5] = Z
    ds = (3, 10, 20, 30, 40, 50, 60)
    at = [128 * s + (6 if s % 2 == 0 else 2) for s in range(7)]   # four in lane half 1, three in half 0: the unsliced merge sees all seven too
    for s, d in enumerate(ds):
        D2[at[s]] = near(kind, Z, d, 30 + s)
    head = [key(d, at[s]) for s, d in enumerate(ds)]
    th = TH[kind]
    dist = P.hamming(D1[[5, 1036, 1037]], D2)
    named = np.zeros(n, bool)
    named[at + list(range(1040, 1046))] = True
    assert dist[:, ~named].min() > th + 5, "the random columns are far from the rows under study"
    exp = dict(cols={5: 6, 1032: 1040, 1035: 1043, 1036: 1044, 1037: 1045, 1040: -1, 0: 0, 1029: 1029}, rescans=2,
               behind_1024=(1032, 1033, 1034, 1035, 1036, 1037), min_live=1085, head_row5={"popcount": head[:4], "mfma": head, "sliced": head})
    z = np.zeros(n, np.float32)
    return Scene("live_behind_1024-%s" % kind, kind, np.ascontiguousarray(D1), np.ascontiguousarray(D2), z, z, 0.6, True, cap, "rescan_take", 1036, (),
                 P.MODELS, exp)


def largest_capacity(kind, cap=4096):
    """cap = 4096, the largest afv_match_bruteforce_pairs_device accepts (PAIR_MAX_SIDE, 16-bit indices in the keys): three copies of B, the
    nearest columns at 4095, 4094, 2048 and 64, so that every index bit of a key is used"""
    D2 = _random_rows(kind, 60000 + nbytes(kind), cap)
    named = {4095: 5, 4094: 20, 2048: 40, 64: 70}
    for v, (q, d) in enumerate(named.items()):
        D2[q] = C(kind, d, 1 + v)
    D1 = np.stack([base_row(kind)] * 3)
    mask = np.ones(cap, bool)
    mask[list(named)] = False
    assert P.hamming(D1[:1], D2)[0, mask].min() > TH[kind] + 5
    head = [key(d, q) for q, d in named.items()]
    exp = dict(head={m: head for m in P.MODELS}, cols={0: 4095, 1: 4094, 2: 2048})
    z1, z2 = np.zeros(3, np.float32), np.zeros(cap, np.float32)
    return Scene("largest_capacity_4096-%s" % kind, kind, np.ascontiguousarray(D1), np.ascontiguousarray(D2), z1, z2, 0.6, True, cap, "keys_accept", 0, (),
                 P.MODELS, exp)


def large_scenes(kind):
    return [live_behind_1024(kind), largest_capacity(kind)]


# ---- tables and calls ----
def table_of(scenes):
    """(table [2 n, cap, bytes] uint8, angles [2 n, cap] float32, counts [2 n]): set 2 i = rows, 2 i + 1 = columns of scene i"""
    cap, nb = scenes[0].cap, scenes[0].D1.shape[1]
    assert all(s.cap == cap and s.D1.shape[1] == nb for s in scenes)
    t = np.zeros((2 * len(scenes), cap, nb), np.uint8)
    a = np.zeros((2 * len(scenes), cap), np.float32)
    n = np.zeros(2 * len(scenes), np.int32)
    for i, s in enumerate(scenes):
        t[2 * i, :len(s.D1)], t[2 * i + 1, :len(s.D2)] = s.D1, s.D2
        a[2 * i, :len(s.D1)], a[2 * i + 1, :len(s.D2)] = s.a1, s.a2
        n[2 * i], n[2 * i + 1] = len(s.D1), len(s.D2)
    return t, a, n


def ratio_groups(scenes):
    """[(ratio, ori, [scene indices])]: what one call can take"""
    groups = collections.OrderedDict()
    for i, s in enumerate(scenes):
        groups.setdefault((s.ratio, s.ori), []).append(i)
    return [(r, o, idx) for (r, o), idx in groups.items()]


def calls_of(scenes, size):
    """[(ratio, ori, [scene index per pair])].  size "chunks": calls of at most 8 pairs (the resolve kernels rescan through L2);
    "all": one call per ratio group, padded with repeats to at least 9 pairs (columns staged in LDS where cap allows it)"""
    out = []
    for ratio, ori, idx in ratio_groups(scenes):
        if size == "chunks":
            out += [(ratio, ori, idx[k:k + 8]) for k in range(0, len(idx), 8)]
        else:
            pad = list(idx)
            while len(pad) < 9:
                pad.append(idx[len(pad) % len(idx)])
            out.append((ratio, ori, pad))
    return out
