"""constructed scenes for the BoW-guided matchers: SearchByBoW(KF, KF), SearchByBoW(KF, F), SearchForTriangulation (test data; no GPU)

Every generator is deterministic (LCG of afv.synth, no global RNG state) and returns Case(name, kind, K1, K2, kw, rule): K1 / K2 are the
FeatureViews the matchers take, kind is "kfkf" / "kff" / "tri", kw the remaining arguments of the oracle binding, `rule` the key of
_bow_ref.FLIPS the scene sits on (None: a structural scene).  tests/test_match_ref_cpu.py proves on the CPU that each scene reaches its rule
and that its outcome depends on it; tests/test_gpu_match_scenes.py runs them through the kernels.

Descriptors are built from DISTANCES with row_at / rows / base_row of _proj_scenes.py: a KF1 row is the base row, a KF2 column the base
with d bits flipped (binary) or an integer offset whose squares sum to d (float: every L2^2 is a small integer).  Rows that must pair up
one to one (the rotation scenes) are `distinct` rows: 2 bits / L2^2 >= 1 apart from each other, 0 from their partner.
(Small integer distances are exact in any summation order: the order of the float distance is tested in tests/_l2_scenes.py.)

Each rule scene comes in three node shapes, one per kernel body behind afv_match_bow:
  single  no FeatureVector (or ONE shared node where the listed order matters)    k_match_bow, or the top-4 + resolve path when eligible
  small   several shared nodes, all at most 64 x 64                                bow_segment_small for binary rows
  large   the scene's node padded to more than 64 on both sides with far-away filler, the filler columns listed FIRST so that the scene's
          columns sit behind bit 64 of the taken flags                              the general bow_segment
Filler rows and columns are further than th_low + 5 from everything (asserted when the scene is built), so they never match.
"""
import collections

import numpy as np

import _bow_ref as R
from _proj_scenes import S, _below, afv, base_row, row_at, rows  # noqa: F401  (afv: the package under test)

f32 = np.float32
Case = collections.namedtuple("Case", "name kind K1 K2 kw rule")

DESCS = ("b32", "b61", "b20", "f8", "f64")
TH = {"b32": 75.0, "b61": 75.0, "b20": 40.0, "f8": 75.0, "f64": 75.0}   # 20-byte rows: random filler sits ~80 bits from anything
SHAPES = ("single", "small", "large")
F_HLINE = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32)   # F12 whose epipolar line of (x1, y1) is y = y1: a = 0, b = 1, c = -y1
FAR_EPIPOLE = (5000.0, 5000.0)
NFILL = 70


def _dist(desc, a, B):
    return (R.l2sqr(a, B) if desc[0] == "f" else R.hamming(a, B)) if len(B) else np.zeros(0, np.float32)


def distinct(desc, i):
    """rows that differ pairwise: base with bit i flipped / base + i along the first dimension"""
    b = base_row(desc).copy()
    if desc[0] == "b":
        assert i < 8 * len(b)
        b[i >> 3] ^= np.uint8(1 << (i & 7))
    else:
        b[0] += f32(i)
    return b


def filler(desc, k, side):
    """row k of the far-away filler of one side"""
    b = base_row(desc).copy()
    if desc[0] == "b":
        return b ^ S.lcg_bytes(9000 + 2 * k + side, len(b))
    b[(3 * k + side) % len(b)] += f32(1000 + k) * (1 if side else -1)
    return b


def _arrays(desc, items, nfill, side, defaults):
    """items: dicts with d / v (distance from the base and variant) or `row` (a ready descriptor) and per-feature attributes"""
    D = [it["row"] if "row" in it else row_at(desc, it.get("d", 0), it.get("v", 0)) for it in items]
    D += [filler(desc, k, side) for k in range(nfill)]
    n = len(D)
    D = np.stack(D) if n else np.zeros((0, len(base_row(desc))), base_row(desc).dtype)
    out = {"desc": np.ascontiguousarray(D)}
    for key, (dflt, dt) in defaults.items():
        present = any(key in it for it in items)
        if key in ("valid", "ur") and not present:
            out[key] = None
            continue
        fill = {"x": 900.0, "y": 900.0, "ur": 5.0}.get(key, dflt)   # filler: off every epipolar line, stereo where stereo matters
        out[key] = np.array([it.get(key, dflt) for it in items] + [fill] * nfill, dt)
    if nfill:
        out["angle"][len(items):] = (S.lcg_states(31 + side, nfill) % 360).astype(np.float32)
    return out


def build(desc, spec, shape):
    """(K1, K2) of one scene in one node shape.  spec: rows, cols, groups = [(indices1, indices2)] the scene's nodes in listed order
    (default: one node holding everything in index order), small_groups = the same for the `small` shape"""
    r_items, c_items = spec["rows"], spec["cols"]
    n1s, n2s = len(r_items), len(c_items)
    groups = spec.get("groups") or [(list(range(n1s)), list(range(n2s)))]
    if shape == "small" and spec.get("small_groups"):
        groups = spec["small_groups"]
    nf1 = nf2 = {"single": 0, "small": 6, "large": NFILL + 6}[shape]
    r = _arrays(desc, r_items, nf1, 0, dict(valid=(1, np.uint8), angle=(0.0, np.float32), x=(100.0, np.float32), y=(50.0, np.float32), ur=(-1.0, np.float32)))
    c = _arrays(desc, c_items, nf2, 1, dict(valid=(1, np.uint8), angle=(0.0, np.float32), x=(200.0, np.float32), y=(50.0, np.float32), s2=(1.0, np.float32),
                                            ur=(-1.0, np.float32)))
    th = spec["kw"].get("th_low", TH[desc])
    if nf1:   # the filler is far from everything
        for i in range(n1s, n1s + nf1):
            assert _dist(desc, r["desc"][i], c["desc"]).min() > th + 5, (desc, shape, "filler row", i)
        for i in range(n1s):
            assert _dist(desc, r["desc"][i], c["desc"][n2s:]).min() > th + 5, (desc, shape, "filler column")
    identity = len(groups) == 1 and groups[0] == (list(range(n1s)), list(range(n2s)))
    if shape == "single":
        fv1 = fv2 = None
        if not identity or spec.get("need_fv"):
            fv1 = [(10 * (k + 1), list(g[0])) for k, g in enumerate(groups)]
            fv2 = [(10 * (k + 1), list(g[1])) for k, g in enumerate(groups)]
    else:
        f1 = list(range(n1s, n1s + nf1)); f2 = list(range(n2s, n2s + nf2))
        fv1 = [(10 * (k + 1), list(g[0])) for k, g in enumerate(groups)]
        fv2 = [(10 * (k + 1), list(g[1])) for k, g in enumerate(groups)]
        if shape == "large":   # half of the filler rows walk before the scene's rows, every filler column is listed before the scene's
            fv1[0] = (10, f1[6:6 + NFILL // 2] + fv1[0][1] + f1[6 + NFILL // 2:])
            fv2[0] = (10, f2[6:] + fv2[0][1])
        # a shared node of filler alone (id 4) and one node per side that the other side does not have (ids 7 and 9999)
        fv1 = [(4, f1[0:3])] + [(7, f1[3:6])] + fv1
        fv2 = [(4, f2[0:3])] + fv2 + [(9999, f2[3:6])]
    K1 = afv.FeatureView(r["desc"], fv1, r["valid"], r["angle"], np.stack([r["x"], r["y"]], 1), None, r["ur"])
    K2 = afv.FeatureView(c["desc"], fv2, c["valid"], c["angle"], np.stack([c["x"], c["y"]], 1), c["s2"], c["ur"])
    return K1, K2


def _cases(name, desc, spec, kinds_rules, shapes=SHAPES):
    out = []
    for shape in shapes:
        K1, K2 = build(desc, spec, shape)
        for kind, rule in kinds_rules:
            kw = dict(spec["kw"])
            kw.setdefault("th_low", TH[desc])
            if kind == "tri":
                kw.setdefault("F12", F_HLINE); kw.setdefault("epipole", FAR_EPIPOLE)
                kw = {k: v for k, v in kw.items() if k in ("th_low", "F12", "epipole", "only_stereo")}
            else:
                kw.setdefault("nnratio", 0.6); kw.setdefault("check_orientation", False)
            out.append(Case("%s-%s-%s-%s" % (name, desc, kind, shape), kind, K1, K2, kw, rule))
    return out


BOTH = lambda rule: (("kfkf", rule), ("kff", rule))


# ---- decision rules of SearchByBoW ----
def bow_rule_scenes(desc):
    th = int(TH[desc])
    row = dict(d=0)
    out = []
    out += _cases("th", desc, dict(rows=[row], cols=[dict(d=th, v=1)], kw=dict(nnratio=0.9)), (("kfkf", "th_lt_kfkf"), ("kff", "th_le_kff")))
    out += _cases("ratio-eq", desc, dict(rows=[row], cols=[dict(d=8, v=1), dict(d=16, v=2)], kw=dict(nnratio=0.5)), BOTH("ratio_lt"))
    # 0.6f * 50.0f = 30.000002: a best distance of 30 is accepted, although 0.6 * 50 is 30
    out += _cases("ratio-f32", desc, dict(rows=[row], cols=[dict(d=30, v=1), dict(d=50, v=2)], kw=dict(nnratio=0.6)), BOTH("ratio_f32"))
    out += _cases("best-first", desc, dict(rows=[row], cols=[dict(d=20, v=3), dict(d=6, v=1), dict(d=6, v=2)], kw=dict(nnratio=1.5)), BOTH("best_first"))
    out += _cases("second", desc, dict(rows=[row], cols=[dict(d=10, v=1), dict(d=38, v=2), dict(d=12, v=3)], kw=dict(nnratio=0.6)), BOTH("second_lt"))
    out += _cases("taken", desc, dict(rows=[row, row], cols=[dict(d=5, v=1), dict(d=20, v=2), dict(d=39, v=3)], kw=dict(nnratio=0.6)), BOTH("taken"))
    out += _cases("valid1", desc, dict(rows=[dict(d=0, valid=0), row], cols=[dict(d=5, v=1), dict(d=30, v=2)], kw={}), BOTH("valid1"))
    # the KF2 mask: honoured by (KF, KF); (KF, F) never looks at a frame-side mask - the same scene, every frame feature masked out, must
    # match as if there were no mask (rule None: the CPU side has nothing to flip, the oracle binding does not even take the argument)
    out += _cases("valid2", desc, dict(rows=[row], cols=[dict(d=5, v=1, valid=0), dict(d=20, v=2)], kw={}), (("kfkf", "valid2"),))
    out += _cases("frame-mask-ignored", desc, dict(rows=[row], cols=[dict(d=5, v=1, valid=0), dict(d=20, v=2, valid=0)], kw={}), (("kff", None),))
    # listed order != index order on both sides: row 1 walks first and takes the near column, which is listed second
    out += _cases("node-order", desc, dict(rows=[row, row], cols=[dict(d=5, v=1), dict(d=20, v=2)], groups=[([1, 0], [1, 0])], kw={}), BOTH("node_order"))
    return out


def merge_scenes(desc):
    """sparse node ids; ids on one side only at the front, in the middle and at the end; nodes with an empty index list.  Every node holds
    one row / one column at distance 0 of each other (distinct code k), so a node joined wrongly or skipped shows in the answer"""
    ids1 = [3, 10, 20, 21, 22, 50, 51, 70, 400, 401]
    ids2 = [1, 2, 10, 21, 23, 24, 50, 52, 70, 90, 400, 9000]
    r_items = [dict(row=distinct(desc, k), angle=10.0 * k) for k in range(len(ids1))]
    codes2 = [ids1.index(i) if i in ids1 else 100 + k for k, i in enumerate(ids2)]
    c_items = [dict(row=distinct(desc, code)) for code in codes2]
    out = []
    for shape in ("small", "large"):
        n1s, n2s = len(r_items), len(c_items)
        nfill = 0 if shape == "small" else NFILL
        r = _arrays(desc, r_items, nfill, 0, dict(valid=(1, np.uint8), angle=(0.0, np.float32), x=(100.0, np.float32), y=(50.0, np.float32), ur=(-1.0, np.float32)))
        c = _arrays(desc, c_items, nfill, 1, dict(valid=(1, np.uint8), angle=(0.0, np.float32), x=(200.0, np.float32), y=(50.0, np.float32),
                                                  s2=(1.0, np.float32), ur=(-1.0, np.float32)))
        fv1 = [(i, [k]) for k, i in enumerate(ids1)]
        fv2 = [(i, [k]) for k, i in enumerate(ids2)]
        fv1[ids1.index(70)] = (70, [])                      # shared id, empty on side 1: its row is in no node
        fv2[ids2.index(400)] = (400, [])                    # shared id, empty on side 2
        if nfill:   # node 21 becomes a large one
            fv1[ids1.index(21)] = (21, list(range(n1s, n1s + nfill)) + [ids1.index(21)])
            fv2[ids2.index(21)] = (21, list(range(n2s, n2s + nfill)) + [ids2.index(21)])
        K1 = afv.FeatureView(r["desc"], fv1, None, r["angle"], np.stack([r["x"], r["y"]], 1), None, None)
        K2 = afv.FeatureView(c["desc"], fv2, None, c["angle"], np.stack([c["x"], c["y"]], 1), c["s2"], None)
        for kind in ("kfkf", "kff"):
            out.append(Case("merge-%s-%s-%s" % (desc, kind, shape), kind, K1, K2, dict(th_low=TH[desc], nnratio=0.6, check_orientation=False), "merge_lower_bound"))
        out.append(Case("merge-%s-tri-%s" % (desc, shape), "tri", K1, K2, dict(th_low=TH[desc], F12=F_HLINE, epipole=FAR_EPIPOLE), "merge_lower_bound"))
    return out


# ---- rotation histogram ----
def _pairs_spec(desc, pairs):
    """pairs: (KF1 angle, other side's angle, copies): row i and the column holding the same descriptor; the columns are stored in
    REVERSE order, so that the index of a match differs between the two sides (the histogram is keyed by one of them)"""
    r_items, c_items = [], []
    for a1, a2, copies in pairs:
        for _ in range(copies):
            i = len(r_items)
            r_items.append(dict(row=distinct(desc, i), angle=a1))
            c_items.append(dict(row=distinct(desc, i), angle=a2))
    n = len(r_items)
    c_items = c_items[::-1]
    small = [(list(range(k, min(k + 16, n))), [n - 1 - i for i in range(k, min(k + 16, n))]) for k in range(0, n, 16)]
    return dict(rows=r_items, cols=c_items, small_groups=small, kw=dict(nnratio=0.6, check_orientation=True))


def rotation_scenes(desc):
    out = []
    half = [a for a in (105.0, 135.0, 165.0, 195.0) if abs(float(f32(a) * (f32(1.0) / f32(30.0)))) % 1.0 == 0.5]
    assert half
    a = half[0]
    k = int(float(f32(a) * (f32(1.0) / f32(30.0))))   # lands in bin k + 1; bin k is a maximum, bin k + 1 is not
    fill = [(0.0, 0.0, 40), (30.0, 0.0, 30), (60.0, 0.0, 20)]
    scenes = [
        ("rot_round", "rot_round", [(0.0, 0.0, 40), (30.0, 0.0, 30), (30.0 * k, 0.0, 20), (a, 0.0, 3)]),
        ("rot_wrap", "rot_wrap", fill + [(900.0, 0.0, 3), (1000.0, 110.0, 2)]),
        ("rot_lt0", "rot_lt0", [(30.0, 0.0, 40), (60.0, 0.0, 30), (90.0, 0.0, 20), (77.0, 77.0, 5), (_below(77.0), 77.0, 4), (200.0, 200.0, 3), (0.0, 0.0, 12)]),
        ("max_first", "max_first", [(0.0, 0.0, 9), (30.0, 0.0, 9), (60.0, 0.0, 9), (90.0, 0.0, 9), (120.0, 0.0, 2)]),
        ("hist_key", "hist_key", [(0.0, 0.0, 9), (30.0, 0.0, 8), (60.0, 0.0, 7), (90.0, 0.0, 5), (120.0, 0.0, 2)]),
    ]
    for m1, m in ((100, 10), (30, 3)):   # (float)max2 / max3 exactly 0.1f * (float)max1
        scenes.append(("max2_lt-%d" % m1, "max2_lt", [(0.0, 0.0, m1), (30.0, 0.0, m), (60.0, 0.0, max(m - 1, 1))]))
        scenes.append(("max3_lt-%d" % m1, "max3_lt", [(0.0, 0.0, m1), (30.0, 0.0, m + 5), (60.0, 0.0, m), (90.0, 0.0, 1)]))
    for name, rule, pairs in scenes:
        out += _cases(name, desc, _pairs_spec(desc, pairs), BOTH(rule))
    return out


# ---- SearchForTriangulation ----
def epiline_edge():
    """(y2, sigma2) with y2 * y2 == 3.84f * sigma2 exactly in float32 (x1' F12 = (0, 1, -y1) with y1 = 0: num = y2, den = 1)"""
    for k in range(4000):
        s2 = f32(1.0) + f32(k) * f32(2.0 ** -12)
        lim = f32(3.84) * s2
        y = np.sqrt(lim, dtype=np.float32)
        for _ in range(3):
            y = _below(y)
        for _ in range(7):
            num = f32(0.0) * f32(200.0) + f32(1.0) * y + f32(-0.0)
            if num * num / f32(1.0) == lim:
                return y, s2
            y = np.nextafter(y, f32(np.inf))
    raise AssertionError("no float32 y2 with y2 * y2 == 3.84f * sigma2")


def tri_rule_scenes(desc):
    th = int(TH[desc])
    row = dict(d=0)          # at (100, 50): its epipolar line is y = 50; columns default to (200, 50), sigma2 = 1
    T = lambda rule: (("tri", rule),)
    out = []
    out += _cases("tri-th", desc, dict(rows=[row], cols=[dict(d=th, v=1)], kw={}), T("tri_th"))
    out += _cases("tri-last", desc, dict(rows=[row], cols=[dict(d=10, v=1), dict(d=10, v=2), dict(d=30, v=3)], kw={}), T("tri_last_wins"))
    # the closer column is off the line: it must not shadow the farther one that is on it
    out += _cases("tri-geom", desc, dict(rows=[row], cols=[dict(d=5, v=1, y=80.0), dict(d=20, v=2)], kw={}), T("tri_geom_before_best"))
    out += _cases("tri-mp1", desc, dict(rows=[dict(d=0, valid=1), dict(d=0, valid=0)], cols=[dict(d=5, v=1, valid=0)], kw={}), T("tri_has_mp1"))
    out += _cases("tri-mp2", desc, dict(rows=[dict(d=0, valid=0)], cols=[dict(d=5, v=1, valid=1), dict(d=20, v=2, valid=0)], kw={}), T("tri_has_mp2"))
    tiny = np.nextafter(f32(0.0), f32(-1.0))    # the largest negative float: monocular
    out += _cases("tri-stereo1", desc, dict(rows=[dict(d=0, ur=u) for u in (0.0, -0.0, tiny, -1.0, 3.0)], cols=[dict(d=5, v=1, ur=5.0)],
                                            kw=dict(only_stereo=True)), T("tri_stereo_ge0"))
    out += _cases("tri-stereo2", desc, dict(rows=[dict(d=0, ur=2.0)], cols=[dict(d=5, v=1, ur=tiny), dict(d=10, v=2, ur=0.0), dict(d=10, v=3, ur=-0.0),
                                                                            dict(d=4, v=4, ur=-7.0)], kw=dict(only_stereo=True)), T("tri_stereo_ge0"))
    out += _cases("tri-only-stereo", desc, dict(rows=[dict(d=0, ur=-1.0), dict(d=0, ur=5.0)], cols=[dict(d=5, v=1, ur=-1.0), dict(d=20, v=2, ur=5.0)],
                                                kw=dict(only_stereo=True)), T("tri_only_stereo"))
    # 30^2 + 40^2 = 2500 = 100.0f * sqrtf(625): not closer than the limit, so kept; the column is on the row's line (sigma2 625 is generous)
    ep = (170.0, 10.0)
    out += _cases("tri-epipole", desc, dict(rows=[row], cols=[dict(d=5, v=1, x=200.0, y=50.0, s2=625.0)], kw=dict(epipole=ep)), T("tri_epipole_lt"))
    # inside the limit, but one side is stereo: the epipole test does not apply
    out += _cases("tri-epipole-stereo", desc, dict(rows=[dict(d=0, ur=4.0), dict(d=0, ur=-1.0)], cols=[dict(d=5, v=1, x=171.0, y=50.0, s2=625.0, ur=-1.0)],
                                                   kw=dict(epipole=(170.0, 50.0))), T("tri_epipole_mono"))
    y2, s2 = epiline_edge()
    out += _cases("tri-epiline", desc, dict(rows=[dict(d=0, x=100.0, y=0.0)], cols=[dict(d=5, v=1, x=200.0, y=float(y2), s2=float(s2)),
                                                                                    dict(d=20, v=2, x=210.0, y=float(_below(y2)), s2=float(s2))], kw={}),
                  T("tri_epiline_lt"))
    out += _cases("tri-den0", desc, dict(rows=[row], cols=[dict(d=5, v=1)], kw=dict(F12=np.zeros(9, np.float32))), T("tri_den0"))
    out += _cases("tri-shared-column", desc, dict(rows=[row, row, row], cols=[dict(d=5, v=1), dict(d=9, v=2)], kw={}), T("tri_not_taken"))
    return out


# ---- structural scenes ----
def chain(desc, n=220):
    """row i sees columns i - 1 and i at distance 1 and every other column at distance 3; row 0 IS column 0.  The first listed of the tie
    (column i - 1) is held by row i - 1, because row i - 2 holds ITS first choice ... down to row 0: every answer depends on the one
    before it.  Without the taken flags each row would meet a tie of best and second and match nothing"""
    base = base_row(desc)
    assert desc[0] == "b" and n <= 8 * len(base)
    cols = [distinct(desc, i) for i in range(n)]
    rws = [cols[0]] + [cols[i] ^ cols[i - 1] ^ base for i in range(1, n)]
    spec = dict(rows=[dict(row=r, angle=0.0) for r in rws], cols=[dict(row=c, angle=0.0) for c in cols], kw=dict(nnratio=0.6))
    return _cases("chain", desc, spec, BOTH(None), ("single", "large"))


def behind(desc, nrow=100, ncol=82):
    """identical rows, columns at distances 0 .. 81: row j ends on the column of rank j, behind j taken ones"""
    spec = dict(rows=[dict(d=0) for _ in range(nrow)], cols=[dict(d=k, v=k) for k in range(ncol)], kw=dict(nnratio=1.0, th_low=75.0))
    return _cases("behind", desc, spec, BOTH(None), ("single", "large"))


def clustered(desc, n1, n2, seed, nodes=None):
    """descriptors a few bits from a set of prototypes (neighbours compete); FeatureVectors: `nodes` = [(id, n1 in node, n2 in node)] dealt in a
    shuffled order, or None"""
    nb = int(desc[1:])
    npro = max(12, max(n1, n2) // 3)   # few enough rows per prototype for the ratio test to leave matches
    rb = lambda sd, m: S.lcg_bytes(sd, max(m, 1) * nb).reshape(max(m, 1), nb)[:m]
    if desc[0] == "b":
        proto = S.lcg_bytes(seed, npro * nb).reshape(npro, nb)
        mk = lambda sd, n, w: proto[w] ^ (rb(sd + 1, n) & rb(sd + 2, n) & rb(sd + 3, n) & rb(sd + 4, n))
    else:
        proto = (S.lcg_states(seed, npro * nb).reshape(npro, nb) % 9).astype(np.float32)
        mk = lambda sd, n, w: (proto[w] + (S.lcg_states(sd + 1, max(n, 1) * nb).reshape(max(n, 1), nb)[:n] % 3).astype(np.float32) - 1)
    w1, w2 = S.lcg_states(seed + 10, n1) % npro, S.lcg_states(seed + 20, n2) % npro
    D1, D2 = np.ascontiguousarray(mk(seed + 10, n1, w1)), np.ascontiguousarray(mk(seed + 20, n2, w2))
    # rows of one prototype share an orientation up to 40 degrees: the histogram has real maxima and real losers
    a1 = ((w1 * 10) % 360 + S.lcg_states(seed + 30, n1) % 40).astype(np.float32)
    a2 = ((w2 * 10) % 360 + S.lcg_states(seed + 31, n2) % 40).astype(np.float32)
    v1 = (S.lcg_bytes(seed + 32, n1) > 25).astype(np.uint8); v2 = (S.lcg_bytes(seed + 33, n2) > 25).astype(np.uint8)
    fv1 = fv2 = None
    if nodes is not None:
        o1 = np.argsort(S.lcg_states(seed + 40, n1), kind="stable"); o2 = np.argsort(S.lcg_states(seed + 41, n2), kind="stable")
        fv1, fv2, p1, p2 = [], [], 0, 0
        for nid, m1, m2 in nodes:
            if m1 is not None:
                fv1.append((nid, o1[p1:p1 + m1].tolist())); p1 += m1
            if m2 is not None:
                fv2.append((nid, o2[p2:p2 + m2].tolist())); p2 += m2
        assert p1 <= n1 and p2 <= n2
    pts1 = np.stack([100.0 + (S.lcg_states(seed + 50, n1) % 400).astype(np.float32), 50.0 + (S.lcg_states(seed + 51, n1) % 4).astype(np.float32)], 1)
    pts2 = np.stack([100.0 + (S.lcg_states(seed + 52, n2) % 400).astype(np.float32), 50.0 + (S.lcg_states(seed + 53, n2) % 4).astype(np.float32)], 1)
    K1 = afv.FeatureView(D1, fv1, v1, a1, pts1.astype(np.float32), None, None)
    K2 = afv.FeatureView(D2, fv2, v2, a2, pts2.astype(np.float32), np.full(n2, 1.44, np.float32), None)
    return K1, K2


def _three(name, desc, K1, K2, kinds=("kfkf", "kff", "tri"), ori=True):
    out = []
    for kind in kinds:
        A, B = K1, K2
        if kind == "tri":   # the masks mean "has a map point" here: one feature in ten has one, not nine
            kw = dict(th_low=TH[desc], F12=F_HLINE, epipole=FAR_EPIPOLE)
            A = afv.FeatureView(K1.descriptors, K1.featvec, None if K1.valid is None else 1 - K1.valid, K1.angles, K1.pts, K1.sigma2, K1.u_right)
            B = afv.FeatureView(K2.descriptors, K2.featvec, None if K2.valid is None else 1 - K2.valid, K2.angles, K2.pts, K2.sigma2, K2.u_right)
        else:
            kw = dict(th_low=TH[desc], nnratio=0.75, check_orientation=ori)
        out.append(Case("%s-%s-%s" % (name, desc, kind), kind, A, B, kw, None))
    return out


def size_scenes():
    out = []
    for desc in ("b32", "b61"):
        for m1 in (63, 64, 65):          # the register-resident form ends at 64 x 64
            for m2 in (63, 64, 65):
                K1, K2 = clustered(desc, m1 + 20, m2 + 20, 300 + m1 * 3 + m2, nodes=[(5, 12, 11), (8, m1, m2), (9, 8, None), (11, None, 9)])
                out += _three("node%dx%d" % (m1, m2), desc, K1, K2, ("kfkf", "kff"))
    for n2 in (31, 32, 33, 2047, 2048, 2049):   # word edges of the taken bitsets
        K1, K2 = clustered("b32", 48, n2, 500 + n2, nodes=[(2, 40, n2 - 6), (6, 8, 6)])
        out += _three("bits%d" % n2, "b32", K1, K2, ("kfkf", "kff"))
    K1, K2 = clustered("f64", 30, 2049, 77, nodes=[(2, 24, 2040), (6, 6, 9)])
    out += _three("bits2049", "f64", K1, K2, ("kfkf", "kff"))
    for n1 in (255, 256, 257):                  # MT = 256 rows per workgroup of k_match_tri; a fifth of the rows sit in no shared node
        K1, K2 = clustered("b32", n1, 300, 600 + n1, nodes=[(1, n1 // 5, None), (3, n1 // 2, 120), (4, n1 - n1 // 5 - n1 // 2, 150), (9, None, 30)])
        out += _three("tri-n%d" % n1, "b32", K1, K2, ("tri",))
    return out


def side_scenes():
    """the largest sides; too slow for the Python loops: these names start with `side-` and carry no rule.  4096 is the last side of the
    top-4 path, 4097 the first that leaves it, 8192 the last the library accepts"""
    out = []
    for n1, n2 in ((4096, 4096), (4097, 300), (300, 4097), (8192, 500), (500, 8192)):
        K1, K2 = clustered("b32", n1, n2, 700 + n1 % 91 + n2 % 89)
        K1.valid = K2.valid = None
        out += _three("side-%dx%d" % (n1, n2), "b32", K1, K2, ("kfkf", "kff") if n1 == n2 else ("kfkf", "kff", "tri"))
    K1, K2 = clustered("b32", 8192, 8192, 801, nodes=[(1, 8000, 8100), (2, 192, 92)])
    out += _three("side-8192-nodes", "b32", K1, K2, ("kfkf",))
    return out


def too_large():
    """8193 on one side: refused, never launched"""
    return clustered("b32", 8193, 40, 811), clustered("b32", 40, 8193, 812)


def all_constructed():
    out = []
    for desc in DESCS:
        out += bow_rule_scenes(desc) + merge_scenes(desc) + rotation_scenes(desc) + tri_rule_scenes(desc)
    out += chain("b32") + chain("b61", 260) + behind("b32") + behind("b61") + size_scenes() + side_scenes()
    return out


def every_route_scene():
    """ONE scene that every route to the BoW-guided kernels can take as it stands (host arrays alone or in a batch, table slots, the table
    against a host frame view and against a RESIDENT frame): its FeatureVectors are what a small vocabulary (k = 5, L = 2, levelsup = 1)
    makes of its descriptors, so Frame::ComputeBoW on the device arrives at K2's.  70 and 65 features of 32 bytes: one full wavefront and a
    ragged tail.  Nodes 1, 2, 3 are shared (25 x 24, 20 x 18, 15 x 15 features), node 4 is on side 1 only (10), node 5 on side 2 only (8);
    the features of a node are scattered over the index range.  Inside a node, feature j of either side sits ~16 bits from sub-prototype
    j (the first six share one between two: they compete), sub-prototypes ~56 bits apart; angles differ by 0 (most), 90 or 200 degrees, so
    the rotation histogram has losers; one feature in ten is masked out on either side.
    Returns (kfkf Case, kff Case, arguments of afv.Vocabulary but ctx)"""
    nb, k = 32, 5
    rnd = lambda sd, m: S.lcg_bytes(sd, max(m, 1) * nb).reshape(max(m, 1), nb)[:m]
    proto = rnd(7001, k)
    sizes = ((25, 24), (20, 18), (15, 15), (10, 0), (0, 8))
    D, A, node = ([], []), ([], []), ([], [])
    for c, ms in enumerate(sizes):
        m = max(ms)
        sub = proto[c] ^ (rnd(7100 + c, m) & rnd(7200 + c, m) & rnd(7300 + c, m))
        which = [j // 2 if j < 6 else j for j in range(m)]
        a1 = (S.lcg_states(7400 + c, m) % 360).astype(np.float32)
        delta = np.choose(S.lcg_states(7500 + c, m) % 20, [200.0] + [90.0] * 3 + [0.0] * 16).astype(np.float32)
        for side in (0, 1):
            n = ms[side]
            sd = 7600 + 10 * c + 5 * side
            D[side].append(sub[which[:n]] ^ (rnd(sd, n) & rnd(sd + 1, n) & rnd(sd + 2, n) & rnd(sd + 3, n)))
            A[side].append((a1[:n] + side * delta[:n]) % np.float32(360.0))
            node[side].extend([c + 1] * n)
    K = []
    for side in (0, 1):
        n = len(node[side])
        order = np.argsort(S.lcg_states(7700 + side, n), kind="stable")
        desc = np.ascontiguousarray(np.concatenate(D[side])[order])
        nid = np.asarray(node[side])[order]
        dist = np.stack([R.hamming(p, desc) for p in proto], 1)            # what the descent at the root compares
        assert np.array_equal(dist.argmin(1) + 1, nid) and np.all(np.sort(dist, 1)[:, 1] - dist.min(1) > 20)
        fv = [(i, np.nonzero(nid == i)[0].tolist()) for i in sorted(set(nid.tolist()))]
        valid = (S.lcg_bytes(7800 + side, n) > 25).astype(np.uint8)
        pts = np.stack([100.0 + 3.0 * np.arange(n), np.full(n, 50.0)], 1).astype(np.float32)
        K.append(afv.FeatureView(desc, fv, valid, np.concatenate(A[side])[order].astype(np.float32), pts, np.ones(n, np.float32), None))
    assert (K[0].N, K[1].N) == (70, 65) and [i for i, _ in K[0].featvec] == [1, 2, 3, 4] and [i for i, _ in K[1].featvec] == [1, 2, 3, 5]
    # the vocabulary: root, 5 nodes at depth 1 (the prototypes, ids 1 .. 5), 5 leaves under each; no stopped word
    parent = [0] + [0] * k + [1 + c for c in range(k) for _ in range(k)]
    leaves = np.concatenate([proto[c] ^ (rnd(7900 + c, k) & rnd(7950 + c, k) & rnd(7990 + c, k)) for c in range(k)])
    node_desc = np.concatenate([np.zeros((1, nb), np.uint8), proto, leaves])
    voc = (k, 2, parent, node_desc, [0.0] + [1.0] * (len(parent) - 1), [False] * (1 + k) + [True] * (k * k))
    kw = dict(th_low=TH["b32"], nnratio=0.75, check_orientation=True)
    return Case("every-route-kfkf", "kfkf", K[0], K[1], kw, None), Case("every-route-kff", "kff", K[0], K[1], dict(kw), None), voc


def zero_shared(desc, seed):
    """FeatureVectors without a common node id"""
    K1, K2 = clustered(desc, 40, 50, seed, nodes=[(1, 20, None), (2, None, 25), (3, 20, None), (4, None, 25)])
    return _three("zero-shared-%d" % seed, desc, K1, K2, ("kfkf", "kff", "tri"))


def batches(cases=None):
    """name -> list of Cases that go into ONE call (kfkf / kff jobs together: the mode is a field of the job; tri jobs in a batch of their
    own).  Every job's answer must be its solo answer."""
    cases = cases if cases is not None else all_constructed()
    by = {c.name: c for c in cases}
    pick = lambda *names: [by[n] for n in names]
    brute = lambda seed, n1, n2, **kw: Case("brute-%d" % seed, "kfkf", *_no_masks(clustered("b32", n1, n2, seed)),
                                            dict(dict(th_low=75.0, nnratio=0.75, check_orientation=True), **kw), None)
    out = collections.OrderedDict()
    out["two-single-and-many"] = pick("taken-b32-kfkf-single", "node64x65-b32-kfkf")
    out["two-zero-and-one"] = [zero_shared("b32", 41)[0], by["node-order-b32-kff-single"]]
    seven = pick("taken-b32-kfkf-single", "node65x64-b61-kff", "ratio-eq-f64-kfkf-small", "chain-b32-kff-single", "merge-b20-kfkf-small",
                 "rot_wrap-b32-kfkf-large", "behind-b61-kfkf-large")
    out["seven-mixed"] = seven + [zero_shared("f8", 43)[1]]
    out["fast-path-settings"] = [brute(901, 300, 280), brute(902, 100, 90), brute(903, 64, 65, th_low=60.0), brute(904, 200, 1, nnratio=0.9),
                                 brute(905, 33, 500, nnratio=0.9), brute(906, 150, 150, check_orientation=False), brute(907, 5, 3, check_orientation=False)]
    out["fast-path-but-one"] = out["fast-path-settings"][:4] + [by["valid1-b32-kfkf-single"]] + out["fast-path-settings"][4:]
    big = []
    names = [c.name for c in cases if c.kind in ("kfkf", "kff") and not c.name.startswith(("side-", "bits2"))]
    for k in range(30):
        big.append(by[names[(k * 37 + 11) % len(names)]])
    out["thirty-three"] = big + [zero_shared("b61", 47)[0], brute(911, 120, 130), by["bits2048-b32-kff"]]
    tri = [c for c in cases if c.kind == "tri" and not c.name.startswith("side-")]
    out["tri-two"] = [by["tri-last-b32-tri-single"], by["tri-n257-b32-tri"]]
    out["tri-seven"] = [tri[(k * 29 + 5) % len(tri)] for k in range(6)] + [zero_shared("b32", 53)[2]]
    out["tri-thirty-three"] = [tri[(k * 31 + 7) % len(tri)] for k in range(32)] + [zero_shared("f64", 59)[2]]
    return out


def _no_masks(pair):
    pair[0].valid = pair[1].valid = None
    return pair


# ---- running a Case through the oracle binding / the restatement ----
def call_args(c):
    K1, K2 = c.K1, c.K2
    if c.kind == "tri":
        return (K1.descriptors, K2.descriptors, K1.pts, K2.pts, K2.sigma2, c.kw["F12"], c.kw["epipole"]), dict(
            nodes1=K1.featvec, nodes2=K2.featvec, has_mp1=K1.valid, has_mp2=K2.valid, th_low=c.kw["th_low"], u_right1=K1.u_right, u_right2=K2.u_right,
            only_stereo=c.kw.get("only_stereo", False))
    kw = dict(th_low=c.kw["th_low"], nnratio=c.kw["nnratio"], check_orientation=c.kw["check_orientation"])
    if c.kind == "kff":
        return (K1.descriptors, K2.descriptors), dict(nodes_kf=K1.featvec, nodes_f=K2.featvec, valid_kf=K1.valid, angle_kf=K1.angles, angle_f=K2.angles, **kw)
    return (K1.descriptors, K2.descriptors), dict(nodes1=K1.featvec, nodes2=K2.featvec, valid1=K1.valid, valid2=K2.valid, angle1=K1.angles,
                                                  angle2=K2.angles, **kw)


FUNCS = {"kfkf": "search_by_bow_kf_kf", "kff": "search_by_bow_kf_frame", "tri": "search_for_triangulation"}


def run_oracle(oracle, c):
    a, kw = call_args(c)
    return getattr(oracle, FUNCS[c.kind])(*a, **kw)


def run_ref(c, flip=None):
    a, kw = call_args(c)
    return getattr(R, FUNCS[c.kind])(*a, flip=flip, **kw)
