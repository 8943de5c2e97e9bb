"""Constructed inputs for vocabulary training (afv_vocab_train against tests/_voctrain_ref.py), built from the project's LCG
(synth.lcg_bytes).  Each scene is small and names the rule it exists for; tests/test_voctrain_ref_cpu.py proves with the restatement's
trace that the rule is reached, tests/test_gpu_voctrain.py holds the device to bit equality on the same scenes.

Sizes the kernels care about (nothing is imported from them): a wavefront is 64 rows, a workgroup pass 256, a tile VT_TILE = 4096 rows
(csrc/afv_voctrain.h) - a node of more rows is worked by several workgroups and finished by a kernel of its own.
"""
import importlib

import numpy as np

import _voctrain_ref as R


def _pkg():
    return importlib.import_module("anyfeature-vslam_amd")


def lcg(seed, n, width):
    return _pkg().synth.lcg_bytes(seed, n * width).reshape(n, width).copy()


def split(rows, pattern):
    """rows -> images of the sizes in `pattern`, cycled (0 = an empty image) until the rows are used up"""
    out, i, p = [], 0, 0
    while i < len(rows):
        m = pattern[p % len(pattern)]
        p += 1
        out.append(rows[i:i + m])
        i += m
    return out


class Scene:
    def __init__(self, name, rule, images, k, L, seed=0, max_iters=0, init_centres=None):
        self.name, self.rule, self.images, self.k, self.L, self.seed, self.max_iters = name, rule, images, k, L, seed, max_iters
        self.init_centres = init_centres
        self.desc_bytes = next(im.shape[1] for im in images if len(im))
        self.n = sum(len(im) for im in images)

    def __repr__(self):
        return self.name


_REF = {}


def ref(scene):
    """(the restatement's answer and trace, computed once per scene and left unchanged)"""
    if scene.name not in _REF:
        trace = R.new_trace()
        out = R.train(scene.images, scene.desc_bytes, scene.k, scene.L, scene.seed, scene.max_iters, scene.init_centres, trace)
        _REF[scene.name] = (out, trace)
    return _REF[scene.name]


def _search_seed(make, wanted, limit=400):
    """the first seed whose trace satisfies `wanted` (the issue: 'find these by searching seeds over 1-byte rows')"""
    for seed in range(limit):
        sc = make(seed)
        trace = R.new_trace()
        R.train(sc.images, sc.desc_bytes, sc.k, sc.L, sc.seed, sc.max_iters, sc.init_centres, trace)
        if wanted(trace):
            return sc
    raise AssertionError("no seed below %d reaches the rule" % limit)


def segment_edges():
    """root sizes around a wavefront (63 / 64 / 65), a workgroup pass (1025) and a tile (4097: the root is a multi-tile node)"""
    return [Scene("edge_n%d" % n, "segment edge", split(lcg(100 + n, n, 32), [50, 7, 0, 31]), 3, 2, seed=n) for n in (63, 64, 65, 1025, 4097)]


def shapes():
    out = []
    for k, L, db, n in ((2, 3, 32, 300), (3, 2, 61, 400), (10, 1, 48, 500), (32, 2, 64, 700), (10, 3, 1, 600), (32, 1, 1, 300), (2, 1, 64, 130),
                        (10, 2, 61, 2000), (3, 3, 48, 257)):
        out.append(Scene("shape_k%d_L%d_b%d" % (k, L, db), "shape", split(lcg(7 * k + L + db, n, db), [64, 1, 100]), k, L, seed=k + L))
    return out


def trivial():
    out = []
    for tag, n in (("n_eq_k", 5), ("n_eq_k_plus_1", 6), ("n_1", 1)):
        out.append(Scene("trivial_" + tag, "trivial case", split(lcg(31 + n, n, 32), [2, 0, 1]), 5, 2, seed=n))
    return out


def deep_multi_tile():
    """two nodes of more than a tile at level 2: multi-tile nodes side by side (their count tables have slots of their own)"""
    return Scene("deep_multi_tile", "multi-tile nodes below the root", split(lcg(77, 9000, 32), [500, 250]), 2, 2, seed=5)


def unbalanced():
    """an early child is a singleton leaf, a later child recurses two more levels: depth-first ids differ from level order"""
    a, b, c = lcg(41, 200, 32), lcg(42, 200, 32), lcg(43, 200, 32)
    base = lcg(44, 3, 32)
    rows = a & b & c                      # sparse noise (an eighth of the bits) ...
    rows[:100] ^= base[0]                 # ... around two blob centres
    rows[100:] ^= base[1]
    rows[17] = base[2]                    # the outlier, far from both
    init = np.stack([rows[17], rows[0], rows[100]])   # (a third child that recurses too: with two, depth-first and level order coincide)
    return Scene("unbalanced", "depth-first ids", split(rows, [40, 0, 25]), 3, 3, seed=3, init_centres=init)


def duplicates():
    """three distinct rows, each repeated many times, k = 5: dist_sum == 0 after three centres, seeding stops short; every image holds all
    three words, so every weight is exactly 0.0 (stopped words); an empty image in the middle and two at the end"""
    base = lcg(51, 3, 32)
    imgs = [np.concatenate([base[[0, 1, 2, 1, 0, 2, 2]]] * 2) for _ in range(6)]
    imgs.insert(3, np.zeros((0, 32), np.uint8))
    imgs += [np.zeros((0, 32), np.uint8), np.zeros((0, 32), np.uint8)]
    return Scene("duplicates", "dist_sum == 0, stopped words, empty images", imgs, 5, 2, seed=9)


def weights_scene():
    """words in some images only; empty images in the middle and at the end of image_ptr"""
    rows = lcg(61, 90, 32)
    imgs = split(rows, [10, 0, 20, 15])
    imgs.append(np.zeros((0, 32), np.uint8))
    return Scene("weights", "TF-IDF over empty images", imgs, 4, 2, seed=2)


def descent_differs():
    """a trivial node (n <= k) with equal rows: each is a cluster of its own in training, the descent sends all of them to the first -
    the later ones are words with Ni == 0 and a feature's descent leaf differs from its training cluster"""
    rows = lcg(71, 5, 32)
    rows[2] = rows[0]
    rows[4] = rows[1]                     # the word of row 1 is in both images: weight log(2 / 2) = 0.0 exactly, a stopped word
    return Scene("descent_differs", "descent leaf != training cluster", [rows[:3], rows[3:]], 5, 1, seed=1)


def majority_ties():
    def make(seed):
        return Scene("majority_ties", "bit count exactly N/2, (N+1)/2, (N-1)/2", split(lcg(200 + seed, 41, 1), [9, 4]), 3, 2, seed=seed)
    return _search_seed(make, lambda t: {(0, 0), (1, 1), (1, -1)} <= t["majority_edge"])


def association_ties():
    def make(seed):
        return Scene("association_ties", "rows equidistant from two centres", split(lcg(300 + seed, 60, 1), [16]), 4, 1, seed=seed)
    return _search_seed(make, lambda t: t["assoc_tie"] > 0)


def seeding_edges():
    def make_a(seed):
        return Scene("seed_cut_boundary", "cut on a running-sum boundary", split(lcg(400 + seed, 9, 1), [4]), 3, 1, seed=seed)

    def make_b(seed):
        return Scene("seed_cut_is_sum", "cut == dist_sum picks the last row with distance left", split(lcg(500 + seed, 7, 1), [4]), 3, 1, seed=seed)
    return [_search_seed(make_a, lambda t: t["cut_on_boundary"] > 0), _search_seed(make_b, lambda t: t["cut_is_sum"] > 0)]


def empty_cluster():
    """init_centres with two equal rows: the second never wins a row (the first minimum stays), stays empty, keeps its centre, and ends as
    a word with Ni == 0"""
    rows = lcg(81, 120, 32)
    rows[:70] = rows[100]                 # most rows equal the doubled centre: its cluster's majority stays that row, the twin never wins one
    init = np.stack([rows[100], rows[100], rows[90]])
    return Scene("empty_cluster", "an empty cluster keeps its centre", split(rows, [30]), 3, 1, seed=4, init_centres=init)


def capped():
    return Scene("max_iters_1", "max_iters = 1 on a scene that needs more rounds", split(lcg(91, 600, 32), [100]), 3, 2, seed=6, max_iters=1)


_ALL = None


def all_constructed():
    global _ALL
    if _ALL is None:
        _ALL = (segment_edges() + shapes() + trivial() + [deep_multi_tile(), unbalanced(), duplicates(), weights_scene(), descent_differs(),
                                                          majority_ties(), association_ties()] + seeding_edges() + [empty_cluster(), capped()])
    return _ALL


def by_name(name):
    return next(s for s in all_constructed() if s.name == name)


def realistic(ctx, nframes=16, per_frame=300):
    """16 synthetic frames through the batch extractor (at most per_frame features each - well under the 500 a frame may bring, to keep the
    restatement at a few seconds), k = 10, L = 3"""
    pkg = _pkg()
    frames = [pkg.synth.corners_frame(900 + i) for i in range(nframes)]
    imgs = []
    for b in range(0, nframes, 8):   # (the test context takes batches of 8)
        imgs += [d[:per_frame].copy() for _, d in ctx.extract_batch(frames[b:b + 8])]
    return Scene("realistic", "extract -> train", imgs, 10, 3, seed=11)
