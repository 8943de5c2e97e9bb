"""GPU: afv_vocab_train / afv_vocab_train_device (Vocabulary.create) against the plain-Python restatement tests/_voctrain_ref.py on the
constructed scenes of tests/_voctrain_scenes.py - bit equality of parent, node descriptors, is_leaf, Ni, the round counts and the weights
(float64 bits), through both entry points (host rows; device rows at a padded pitch)."""
import ctypes as C
import threading

import numpy as np
import pytest

import _voctrain_ref as R
import _voctrain_scenes as S

pytestmark = pytest.mark.gpu
CASES = S.all_constructed()


def train_gpu(afv, ctx, sc, entry="host", seed=None):
    seed = sc.seed if seed is None else seed
    if entry == "host":
        return afv.Vocabulary.create(sc.images, sc.k, sc.L, seed, ctx, sc.max_iters, sc.init_centres)
    import torch
    pitch = 64 if sc.desc_bytes <= 48 else 80        # padded rows, the padding filled with ones: it must not count
    rows = np.full((sc.n, pitch), 255, np.uint8)
    rows[:, :sc.desc_bytes] = np.concatenate([im for im in sc.images if len(im)])
    iptr = np.zeros(len(sc.images) + 1, np.int32)
    iptr[1:] = np.cumsum([len(im) for im in sc.images])
    t = torch.from_numpy(rows).cuda()
    return afv.Vocabulary.create(t, sc.k, sc.L, seed, ctx, sc.max_iters, sc.init_centres, image_ptr=iptr, pitch=pitch, desc_bytes=sc.desc_bytes)


def tree_of(v):
    st = v.train_stats
    return (st["parent"].tolist(), v.node_desc.tobytes(), v.is_leaf.tolist(), st["ni"].tolist(), st["rounds"].tolist(), v.weight.tobytes(), st["capped"])


def check_against_ref(sc, v):
    out, _ = S.ref(sc)
    st = v.train_stats
    assert st["parent"].tolist() == out["parent"]
    assert v.is_leaf.tolist() == out["is_leaf"]
    assert v.node_desc.shape == (len(out["parent"]), sc.desc_bytes)
    got = [bytes(r) for r in v.node_desc]
    assert got == out["desc"]
    assert st["ni"].tolist() == out["ni"]
    assert st["rounds"].tolist() == out["rounds"]
    assert st["capped"] == out["capped"]
    assert v.weight.tobytes() == np.asarray(out["weight"], np.float64).tobytes()
    assert (v.k, v.L) == (sc.k, sc.L)


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("sc", CASES, ids=repr)
def test_scene_bit_equal(afv, gpu_ctx, sc, entry):
    check_against_ref(sc, train_gpu(afv, gpu_ctx, sc, entry))


def test_realistic_scene(afv, gpu_ctx):
    sc = S.realistic(gpu_ctx)
    assert sc.n > 4096 and len(sc.images) == 16
    check_against_ref(sc, train_gpu(afv, gpu_ctx, sc, "host"))
    check_against_ref(sc, train_gpu(afv, gpu_ctx, sc, "device"))


def test_same_seed_same_tree_other_seed_other_tree(afv, gpu_ctx):
    sc = S.by_name("shape_k10_L2_b61")
    a, b, c = train_gpu(afv, gpu_ctx, sc), train_gpu(afv, gpu_ctx, sc), train_gpu(afv, gpu_ctx, sc, seed=sc.seed + 1)
    assert tree_of(a) == tree_of(b)
    assert tree_of(a) != tree_of(c)


def test_trained_vocabulary_is_an_ordinary_one(afv, gpu_ctx, tmp_path):
    sc = S.by_name("shape_k10_L2_b61")
    v = train_gpu(afv, gpu_ctx, sc)
    path = str(tmp_path / "trained.txt")
    v.saveToTextFile(path)
    w = afv.Vocabulary.loadFromTextFile(path, gpu_ctx)
    q = S.lcg(999, 300, sc.desc_bytes)
    lv, nv = v.transform_nodes(q, 1)
    lw, nw = w.transform_nodes(q, 1)
    assert np.array_equal(lv, lw) and np.array_equal(nv, nw)
    out, _ = S.ref(sc)
    rows = [int.from_bytes(bytes(r), "little") for r in q]
    assert lv.tolist() == [R.descend(r, out["desc_int"], out["children"]) for r in rows]
    wv, vv = v.bow_vector(lv)
    ww, vw = w.bow_vector(lw)
    assert np.array_equal(wv, ww) and vv.tobytes() == vw.tobytes() and len(wv) > 0
    assert v.transform(q, 1) == w.transform(q, 1)
    v.close(); w.close()
    # a resident frame's ComputeBoW accepts a trained 32-byte vocabulary
    sc32 = S.by_name("shape_k2_L3_b32")
    v32 = train_gpu(afv, gpu_ctx, sc32)
    desc = S.lcg(998, 200, 32)
    kps = np.zeros(200, afv.KP_DTYPE)
    kps["x"], kps["y"], kps["size"] = np.arange(200) % 600 + 10, np.arange(200) % 400 + 10, 31.0
    fr = afv.Frame(gpu_ctx)
    fr.set_features(kps, desc)
    assert fr.ComputeBoW(v32, 1) == v32.transform(desc, 1)
    fr.close(); v32.close()


def test_limits_answer_einval(afv, gpu_ctx):
    L = afv._lib
    lib = L.load()
    rows = S.lcg(5, 100, 32)
    iptr = np.array([0, 40, 100], np.int32)

    def call(k=3, Lv=2, db=32, n=100, ip=iptr, nimg=2, n_init=0, init=None, size=None, device=False):
        prm = L.sized(L.VocabTrainParams)
        prm.k, prm.L, prm.desc_bytes, prm.n_init = k, Lv, db, n_init
        prm.init_centres = init.ctypes.data if init is not None else None
        if size is not None:
            prm.struct_size = size
        out = C.c_void_p(12345)
        if device:
            rc = lib.afv_vocab_train_device(gpu_ctx.handle, C.byref(prm), L.ptr(rows), 16, n, L.ptr(ip), nimg, C.byref(out))   # pitch < desc_bytes
        else:
            rc = lib.afv_vocab_train(gpu_ctx.handle, C.byref(prm), L.ptr(rows), n, L.ptr(ip), nimg, C.byref(out))
        return rc, out.value

    bad = [dict(k=1), dict(k=33), dict(Lv=0), dict(Lv=11), dict(db=0), dict(db=65), dict(n=0, ip=np.array([0, 0, 0], np.int32)),
           dict(n=L.VOCAB_TRAIN_MAX_ROWS + 1, ip=np.array([0, 40, L.VOCAB_TRAIN_MAX_ROWS + 1], np.int32)),
           dict(ip=np.array([1, 40, 100], np.int32)), dict(ip=np.array([0, 101, 100], np.int32)), dict(ip=np.array([0, 40, 99], np.int32)),
           dict(nimg=0), dict(n_init=4, init=rows[:4]), dict(n_init=2), dict(size=8), dict(device=True)]
    for kw in bad:
        rc, out = call(**kw)
        assert rc == L.EINVAL and not out, kw
    rc, out = call()
    assert rc == L.OK and out
    assert lib.afv_vocab_tree_nnodes(C.c_void_p(out)) > 3
    lib.afv_vocab_tree_destroy(C.c_void_p(out))


def test_two_contexts_on_two_threads(afv, gpu_ctx):
    """the reference calls the library from three threads: two trainings, each on a context of its own, give the single-thread trees"""
    scenes = [S.by_name("shape_k10_L2_b61"), S.by_name("edge_n4097")]
    want = [tree_of(train_gpu(afv, gpu_ctx, sc)) for sc in scenes]
    ctxs = [afv.Context(), afv.Context()]
    got, errors = [None, None], []

    def work(i):
        try:
            for _ in range(2):
                got[i] = tree_of(train_gpu(afv, ctxs[i], scenes[i], "host" if i == 0 else "device"))
        except Exception as e:  # noqa: BLE001 - reported below, on the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert got == want
