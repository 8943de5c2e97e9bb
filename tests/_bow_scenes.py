"""Seeded place-recognition scenes for the BowVector / score tests (no files): a Vocabulary.random tree with 10 000 words (k = 10, L = 4;
with the 216 words of the default tree every pair of keyframes shares nearly every word and the gates of KeyFrameDatabase never bite)
and a run of keyframes that visits a few "places" twice.  A keyframe copies part of its descriptors from its place's pool, the rest is
its own, so the scores between keyframes spread.

The leaves of every descriptor are worked out here on the CPU (numpy, first minimum wins like the device descent), so the conditions a
scene must meet can be asserted without a GPU (tests/test_kfdb_ref_cpu.py); the GPU tests check that the device descent returns the same
leaves before they rely on them."""
import importlib

import numpy as np

KINDS = {"orb32": dict(desc_bytes=32, float_dim=0), "akaze61": dict(desc_bytes=61, float_dim=0), "sift128": dict(desc_bytes=512, float_dim=128)}
K_TREE, L_TREE = 10, 4
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
_cache = {}


def _pkg():
    return importlib.import_module("anyfeature-vslam_amd")


def vocabulary(kind, ctx=None):
    """a fresh Vocabulary object of the scene's tree (the arrays are the same for every call)"""
    afv = _pkg()
    spec = KINDS[kind]
    if spec["float_dim"]:
        return afv.Vocabulary.random_float(11, K_TREE, L_TREE, ctx, dim=spec["float_dim"])
    return afv.Vocabulary.random(11, K_TREE, L_TREE, ctx, desc_bytes=spec["desc_bytes"])


def cpu_leaves(voc, desc):
    """the descent of k_bow.hip on the CPU: at every level the nearest child, first minimum wins"""
    desc = np.asarray(desc)
    n = len(desc)
    cur = np.zeros(n, np.int64)
    rows = np.arange(n)
    for _ in range(voc.L):
        kids = voc.child_idx[voc.child_ptr[cur][:, None] + np.arange(voc.k)[None, :]]          # complete tree: k children everywhere
        if voc.is_float:
            d = desc[:, None, :].astype(np.float32) - voc.node_desc[kids]
            dist = np.cumsum((d * d).astype(np.float64), axis=-1)[..., -1]                        # float squares, double sum in index order
        else:
            dist = _POP[desc[:, None, :] ^ voc.node_desc[kids]].sum(-1)
        cur = kids[rows, np.argmin(dist, axis=1)].astype(np.int64)
    return cur.astype(np.int32)


def _descriptors(kind, rng, n):
    spec = KINDS[kind]
    if spec["float_dim"]:
        d = rng.randint(0, 256, (n, spec["float_dim"])).astype(np.float32) ** 2
        return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return rng.randint(0, 256, (n, spec["desc_bytes"])).astype(np.uint8)


class Scene:
    """keyframes[i]: descriptors of keyframe i (= table slot i); leaves[i]: their leaf nodes; place[i]; covis: GetBestCovisibilityKeyFrames;
    frame_desc / frame_leaves: the relocalisation query; loop_slot / connected: the loop query"""

    def best_covisibles(self, slot):
        return self.covis.get(int(slot), [])


def scene(kind, nkf=96, nplaces=6, run=8, seed=5):
    key = (kind, nkf, nplaces, run, seed)
    if key in _cache:
        return _cache[key]
    rng = np.random.RandomState(seed)
    voc = vocabulary(kind)
    pools = [_descriptors(kind, rng, 600) for _ in range(nplaces)]
    s = Scene()
    s.kind, s.nkf, s.weight, s.word_id = kind, nkf, voc.weight, voc.word_id
    s.keyframes, s.place = [], []

    def view_of(place, n, frac):
        ncopy = int(n * frac)
        own = _descriptors(kind, rng, n - ncopy)
        d = np.concatenate([pools[place][rng.choice(600, ncopy, replace=False)], own])
        return np.ascontiguousarray(d[rng.permutation(n)])

    for i in range(nkf):
        p = (i // run) % nplaces
        s.place.append(p)
        # a few overlap classes: keyframes of the upper ones come within 80 % of the best common-word count, the others do not
        frac = 0.9 if i == nkf - 1 else (0.3, 0.5, 0.8, 0.85, 0.9, 0.95)[rng.randint(6)]
        s.keyframes.append(view_of(p, int(rng.randint(400, 461)), frac))
    # covisibility: neighbours of the same run, nearest first; every fifth keyframe has none (its accumulated score stays its own)
    s.covis = {}
    for i in range(nkf):
        if i % 5 == 0:
            continue
        near = sorted((j for j in range(max(0, i - 4), min(nkf, i + 5)) if j != i and j // run == i // run), key=lambda j: (abs(j - i), j))
        s.covis[i] = near[:10]
    s.leaves = [cpu_leaves(voc, d) for d in s.keyframes]
    # relocalisation: a new view of place 2
    s.frame_place = 2
    s.frame_desc = view_of(2, 450, 0.8)
    s.frame_leaves = cpu_leaves(voc, s.frame_desc)
    # loop closing: the last keyframe queries; the keyframes of its own run are connected to it, its place was seen one round earlier
    s.loop_slot = nkf - 1
    s.connected = [j for j in range(nkf - 1) if j // run == (nkf - 1) // run]
    _cache[key] = s
    return s
