"""GPU: afv_frame_initializer (include/afv_hip.h, "Initializer"; csrc/k_init.hip) against the restatement tests/_init_ref.py, bit for bit:
ok, route, R21, t21, p3d, triangulated, the trace and every per-hypothesis array, for every constructed scene of tests/_init_scenes.py;
frames of every descriptor kind; a frame whose mvKeysUn came through set_undistorted; every refusal with the outputs untouched; the Python
class against the C call; seeds."""
import ctypes as C

import numpy as np
import pytest

import _init_scenes as S
from _init_check import check_against, same

pytestmark = pytest.mark.gpu


def make_frame(afv, ctx, x, y, kind="orb32", undistorted=False):
    """a resident frame whose mvKeysUn are (x, y)"""
    n = len(x)
    kw = dict(orb32={}, akaze61=dict(desc_bytes=61), sift128=dict(float_dim=128))[kind]
    fr = afv.Frame(ctx, min_x=-4000.0, min_y=-4000.0, max_x=4000.0, max_y=4000.0, distorted=undistorted, **kw)
    rng = np.random.default_rng(n)
    kps = np.zeros(n, afv.KP_DTYPE)
    if undistorted:   # the distorted positions are something else entirely
        kps["x"], kps["y"] = rng.uniform(0, 640, n), rng.uniform(0, 480, n)
    else:
        kps["x"], kps["y"] = x, y
    desc = rng.random((n, 128), dtype=np.float32) if kind == "sift128" else rng.integers(0, 256, (n, fr.desc_bytes), dtype=np.uint8)
    fr.set_features(kps, desc, sizes=np.ones(n, np.float32))
    if undistorted:
        fr.set_undistorted(x, y)
    return fr


def job_of(afv, sc, iterations=None, seed=None):
    j = afv._lib.sized(afv._lib.InitJob)
    j.iterations = sc.iterations if iterations is None else iterations
    seed = (sc.seed if seed is None else seed) & 0xFFFFFFFFFFFFFFFF
    j.seed_lo, j.seed_hi = seed & 0xFFFFFFFF, seed >> 32
    j.fx, j.fy, j.cx, j.cy, j.sigma = float(sc.fx), float(sc.fy), float(sc.cx), float(sc.cy), float(sc.sigma)
    return j


def call(afv, ctx, sc, kind="orb32", undistorted=False, **kw):
    f1 = make_frame(afv, ctx, sc.x1, sc.y1, kind, undistorted)
    f2 = make_frame(afv, ctx, sc.x2, sc.y2, kind, undistorted)
    try:
        return afv.initializer.initialize(f1, f2, job_of(afv, sc), sc.matches12, hypotheses=True, **kw)
    finally:
        f1.close()
        f2.close()


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_scene_is_bit_equal_to_the_restatement(afv, gpu_ctx, name):
    sc = S.scene(name)
    check_against(call(afv, gpu_ctx, sc), S.reference(name), sc, name)


@pytest.mark.parametrize("kind", ["akaze61", "sift128"])
def test_descriptor_kind_and_width_do_not_matter(afv, gpu_ctx, kind):
    for name in ("cloud", "plane"):
        sc = S.scene(name)
        check_against(call(afv, gpu_ctx, sc, kind=kind), S.reference(name), sc, "%s %s" % (kind, name))


def test_keys_that_came_through_set_undistorted(afv, gpu_ctx):
    sc = S.scene("outliers")
    check_against(call(afv, gpu_ctx, sc, undistorted=True), S.reference("outliers"), sc, "undistorted")


def test_mask_words_wider_than_needed_are_zero_padded(afv, gpu_ctx):
    sc = S.scene("n65")
    got = call(afv, gpu_ctx, sc, mask_words=7)
    assert got["inliers"].shape[2] == 7 and not got["inliers"][:, :, 3:].any() and got["inliers"][:, :, 2].any()
    check_against(got, S.reference("n65"), sc, "mask_words 7")


def test_refusals_leave_the_outputs_untouched(afv, gpu_ctx):
    L = afv._lib
    lib = L.load()
    sc = S.scene("n65")
    f1, f2 = make_frame(afv, gpu_ctx, sc.x1, sc.y1), make_frame(afv, gpu_ctx, sc.x2, sc.y2)
    other = afv.Context(max_width=640, max_height=480, max_batch=1)
    foreign = make_frame(afv, other, sc.x2, sc.y2)
    raw = afv.Frame(gpu_ctx, distorted=True)
    kps = np.zeros(len(sc.x2), afv.KP_DTYPE)
    raw.set_features(kps, np.zeros((len(kps), 32), np.uint8), sizes=np.ones(len(kps), np.float32))   # no set_undistorted yet
    n1, it, mw = len(sc.x1), sc.iterations, 3
    try:
        def attempt(f1h=f1.handle, f2h=f2.handle, job=None, matches=sc.matches12, drop=(), mask_words=mw, trace_size=None, **fields):
            j = job_of(afv, sc) if job is None else job
            for k, v in fields.items():
                setattr(j, k, v)
            out = dict(ok=np.full(1, 0x5A5A5A5A, np.int32), route=np.full(1, 0x5A5A5A5A, np.int32), R21=np.full(9, 7.5, np.float32),
                       t21=np.full(3, 7.5, np.float32), p3d=np.full((n1, 3), 7.5, np.float32), tri=np.full(n1, 0x5A, np.uint8),
                       score=np.full((2, it), 7.5, np.float32), model=np.full((2, it, 9), 7.5, np.float32), deg=np.full((2, it), 0x5A, np.uint8),
                       inl=np.full((2, it, max(mask_words, 1)), 0x5A5A5A5A, np.uint32))
            tr = L.sized(L.InitTrace)
            if trace_size is not None:
                tr.struct_size = trace_size
            tr.n = 0x5A5A
            before = {k: v.copy() for k, v in out.items()}
            p = {k: (None if k in drop else L.ptr(v)) for k, v in out.items()}
            m = np.ascontiguousarray(matches, np.int32)
            code = lib.afv_frame_initializer(f1h, f2h, None if "job" in drop else C.byref(j), None if "matches" in drop else L.ptr(m),
                                             C.cast(p["ok"], C.POINTER(C.c_int32)), C.cast(p["route"], C.POINTER(C.c_int32)), p["R21"], p["t21"],
                                             p["p3d"], p["tri"], C.byref(tr), p["score"], p["model"], p["deg"], p["inl"], mask_words)
            untouched = all(np.array_equal(out[k], before[k]) for k in out) and tr.n == 0x5A5A
            return code, untouched

        assert attempt() == (L.OK, False)
        for drop in ("ok", "route", "R21", "t21", "p3d", "tri", "job", "matches"):
            assert attempt(drop=(drop,)) == (L.EINVAL, True), drop
        assert attempt(f1h=None) == (L.EINVAL, True) and attempt(f2h=None) == (L.EINVAL, True)
        assert attempt(f2h=foreign.handle) == (L.EINVAL, True)           # frames of different contexts
        assert attempt(f2h=raw.handle) == (L.EINVAL, True)               # a distorted frame that has no mvKeysUn yet
        for bad in (0, -1, L.INIT_MAX_ITERATIONS + 1):
            assert attempt(iterations=bad) == (L.EINVAL, True), bad
        assert attempt(iterations=L.INIT_MAX_ITERATIONS + 1)[0] == L.EINVAL
        for size in (0, 4, 35, 4 * C.sizeof(L.InitJob) + 4):
            assert attempt(struct_size=size) == (L.EINVAL, True), size
        assert attempt(trace_size=C.sizeof(L.InitTrace) - 4) == (L.EINVAL, True)
        for value in (-2, len(sc.x2), 1 << 30):
            m = sc.matches12.copy()
            m[int(np.argmax(m >= 0))] = value
            assert attempt(matches=m) == (L.EINVAL, True), value
        for field in ("sigma", "fx", "fy"):
            for value in (0.0, -1.0, float("nan"), float("inf")):
                assert attempt(**{field: value}) == (L.EINVAL, True), (field, value)
        assert attempt(mask_words=2) == (L.EINVAL, True)                 # 64 bits for 65 matches
        assert attempt(mask_words=-1) == (L.EINVAL, True) and attempt(mask_words=L.INIT_MAX_MASK_WORDS + 1) == (L.EINVAL, True)
        assert attempt(mask_words=2, drop=("inl",)) == (L.OK, False)     # no inlier rows asked for: any width
    finally:
        for f in (f1, f2, foreign, raw):
            f.close()
        other.close()


def test_python_class_against_the_c_call(afv, gpu_ctx):
    sc = S.scene("cloud")
    want = S.reference("cloud")
    f1, f2 = make_frame(afv, gpu_ctx, sc.x1, sc.y1), make_frame(afv, gpu_ctx, sc.x2, sc.y2)
    try:
        K = np.array([[sc.fx, 0, sc.cx], [0, sc.fy, sc.cy], [0, 0, 1]], np.float32)
        ini = afv.Initializer(f1, K, float(sc.sigma), sc.iterations)
        ok, R21, t21, p3d, tri = ini.Initialize(f2, sc.matches12, seed=sc.seed, hypotheses=True)
        raw = afv.initializer.initialize(f1, f2, job_of(afv, sc), sc.matches12, hypotheses=True)
        assert ok is True and raw["ok"] == 1 and want["ok"] == 1 and tri.dtype == bool
        same(R21.reshape(9), raw["R21"], "R21")
        same(t21, raw["t21"], "t21")
        same(p3d, raw["p3d"], "p3d")
        same(tri.astype(np.uint8), raw["triangulated"], "triangulated")
        for k, v in ini.hypotheses().items():
            same(v, raw[k], k)
        assert bytes(ini.trace) == bytes(raw["trace"]) and ini.trace.reason == 0
        deg = ini.parallax_degrees()
        assert len(deg) == 4 and deg[ini.trace.best_motion] > 1.0
        four = afv.Initializer(f1, (sc.fx, sc.fy, sc.cx, sc.cy), float(sc.sigma), sc.iterations)
        assert four.Initialize(f2, sc.matches12, seed=sc.seed)[0] is True and bytes(four.trace) == bytes(ini.trace)
        with pytest.raises(RuntimeError):
            four.hypotheses()
        with pytest.raises(ValueError):
            ini.Initialize(f2, sc.matches12[:-1])
    finally:
        f1.close()
        f2.close()


def test_seeds(afv, gpu_ctx):
    sc = S.scene("outliers")
    f1, f2 = make_frame(afv, gpu_ctx, sc.x1, sc.y1), make_frame(afv, gpu_ctx, sc.x2, sc.y2)
    try:
        run = lambda seed: afv.initializer.initialize(f1, f2, job_of(afv, sc, seed=seed), sc.matches12, hypotheses=True)
        a, b, c = run(11), run(11), run((1 << 40) + 11)
        for k in ("score", "model", "degenerate", "inliers"):
            same(a[k], b[k], k)
        assert bytes(a["trace"]) == bytes(b["trace"])
        assert not np.array_equal(a["score"], c["score"]) and not np.array_equal(a["model"], c["model"])
    finally:
        f1.close()
        f2.close()
