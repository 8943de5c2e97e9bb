"""-m gpu: afv_table_sim3_hypotheses (csrc/k_sim3.hip) against the restatement (tests/_sim3_ref.py), bit for bit: every output array,
float bits included, the optional x3dc / max_err outputs, and the iterate / find traces of the Python class.  Shapes: N at the wavefront
and mask-word edges, nhyp around the workgroup's four wavefronts, batches against their candidates one by one, n1 on both sides of the
gather workgroup, minimal and generous mask_words, the three table kinds, a cloned table, a slot promoted from a frame, every error
answer with the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

import _sim3_ref as R
import _sim3_scenes as S

pytestmark = pytest.mark.gpu
KEYS = ("n", "index1", "count", "degenerate", "sim3", "inliers", "x3dc1", "x3dc2", "max_err")
_cache = {}


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class Rig:
    """scenes installed in a table (scene c: slots 2c and 2c + 1) and a store (scene c: ids from base[c] on)"""

    def __init__(self, afv, ctx, scenes, cap, desc_bytes=32, float_dim=0, spare=3):
        self.afv, self.ctx, self.scenes, self.cap = afv, ctx, scenes, cap
        kind = {"float_dim": float_dim} if float_dim else {"desc_bytes": desc_bytes}
        self.table = afv.table.DescriptorTable(ctx, 2 * len(scenes), cap, **kind)
        self.base = np.cumsum([0] + [len(sc.pos) for sc in scenes])
        self.points = afv.MapPoints(ctx, int(self.base[-1]) + spare, **kind)
        rng = np.random.default_rng(4)
        for c, sc in enumerate(scenes):
            for slot, n, sig in ((2 * c, sc.n1, sc.sigma2_1), (2 * c + 1, sc.n2, sc.sigma2_2)):
                rows = rng.normal(0, 1, (n, float_dim)).astype(np.float32) if float_dim else rng.integers(0, 256, (n, desc_bytes), dtype=np.uint8)
                self.table.set(slot, rows)
                self.table.set_geometry(slot, rng.uniform(0, 640, n), rng.uniform(0, 480, n), sig)
            ids = np.nonzero(sc.flags & R.SET)[0].astype(np.int32)
            if len(ids):
                self.points.set(ids + self.base[c], pos=sc.pos[ids])
                self.points.set_flags(ids + self.base[c], bad=(sc.flags[ids] & R.BAD) != 0)

    def close(self):
        self.points.close()
        self.table.close()

    def rows(self, which=None):
        """mp1, mp2, idx1 (None when no scene carries one), idx2 as [nc, cap] with the store's id bases applied"""
        sel = range(len(self.scenes)) if which is None else which
        out = {k: np.full((len(sel), self.cap), -1, np.int32) for k in ("mp1", "mp2", "idx1", "idx2")}
        any_idx1 = any(self.scenes[c].idx1 is not None for c in sel)
        for r, c in enumerate(sel):
            sc = self.scenes[c]
            for k in ("mp1", "mp2"):
                v = getattr(sc, k)
                out[k][r, :sc.n1] = np.where(v >= 0, v + self.base[c], -1)
            out["idx2"][r, :sc.n1] = sc.idx2
            out["idx1"][r, :sc.n1] = np.arange(sc.n1) if sc.idx1 is None else sc.idx1
        return out["mp1"], out["mp2"], (out["idx1"] if any_idx1 else None), out["idx2"]

    def jobs(self, which=None):
        sel = range(len(self.scenes)) if which is None else which
        L = self.afv._lib
        jobs = (L.Sim3Job * len(sel))()
        for r, c in enumerate(sel):
            sc, j = self.scenes[c], jobs[r]
            j.struct_size, j.fix_scale = C.sizeof(L.Sim3Job), int(sc.fix_scale)
            j.seed_lo, j.seed_hi = sc.seed & 0xFFFFFFFF, (sc.seed >> 32) & 0xFFFFFFFF
            for side, cam in (("1", sc.cam1), ("2", sc.cam2)):
                for k in range(9):
                    getattr(j, "Rcw" + side)[k] = float(cam.Rcw[k])
                for k in range(3):
                    getattr(j, "tcw" + side)[k] = float(cam.tcw[k])
                for key in ("fx", "fy", "cx", "cy"):
                    setattr(j, key + side, float(getattr(cam, key)))
        return jobs

    def outputs(self, nc, nhyp, mask_words, poison=0xA5):
        shapes = dict(n=((nc,), np.int32), index1=((nc, self.cap), np.int32), count=((nc, nhyp), np.int32), degenerate=((nc, nhyp), np.uint8),
                      sim3=((nc, nhyp, 13), np.float32), inliers=((nc, nhyp, mask_words), np.uint32), x3dc1=((nc, self.cap, 3), np.float32),
                      x3dc2=((nc, self.cap, 3), np.float32), max_err=((nc, self.cap, 2), np.float32))
        out = {}
        for k, (shape, dt) in shapes.items():
            out[k] = np.zeros(shape, dt)
            raw(out[k])[:] = poison
        return out

    def call(self, nhyp, mask_words, which=None, table=None, points=None, out=None, **over):
        """the C entry point as it is: returns (code, outputs).  Outputs start poisoned: what the call leaves is what it wrote"""
        sel = list(range(len(self.scenes))) if which is None else list(which)
        nc = len(sel)
        mp1, mp2, idx1, idx2 = self.rows(sel)
        a = dict(slot_a=np.array([2 * c for c in sel], np.int32), slot_b=np.array([2 * c + 1 for c in sel], np.int32), jobs=self.jobs(sel), nc=nc,
                 mp1=mp1, mp2=mp2, idx1=idx1, idx2=idx2, nhyp=nhyp, mask_words=mask_words)
        a.update(over)
        out = out or self.outputs(nc, max(nhyp, 1), max(mask_words, 0))
        p = self.afv._lib.ptr
        t = (table or self.table).handle
        s = (points or self.points).handle
        code = self.table.lib.afv_table_sim3_hypotheses(
            t, s, p(a["slot_a"]), p(a["slot_b"]), a["jobs"], a["nc"], p(a["mp1"]), p(a["mp2"]), p(a["idx1"]), p(a["idx2"]), a["nhyp"],
            a["mask_words"], *[p(out[k]) for k in KEYS])
        return code, out

    def want(self, nhyp, mask_words, which=None, key=None):
        sel = range(len(self.scenes)) if which is None else which
        per = [cached((key, c, self.cap, nhyp, mask_words), lambda c=c: self.scenes[c].candidate(self.cap, nhyp, mask_words)) if key else
               self.scenes[c].candidate(self.cap, nhyp, mask_words) for c in sel]
        return {k: np.stack([np.asarray(w[k]) for w in per]) for k in KEYS}, per


def assert_same(got, want, name):
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k]).astype(got[k].dtype)
        assert g.shape == w.shape, (name, k, g.shape, w.shape)
        if raw(g).tobytes() != raw(w).tobytes():
            bad = np.argwhere(g.view(np.uint32 if g.dtype.itemsize == 4 else np.uint8) != w.view(np.uint32 if w.dtype.itemsize == 4 else np.uint8))
            raise AssertionError("%s: %s differs at %s: got %r, want %r" % (name, k, bad[0], g[tuple(bad[0])], w[tuple(bad[0])]))


def words_for(n):
    return (n + 31) // 32


def run(afv, ctx, scenes, cap, nhyp, mask_words, key, **kind):
    rig = Rig(afv, ctx, scenes, cap, **kind)
    try:
        code, got = rig.call(nhyp, mask_words)
        assert code == 0, afv._lib.strerror(code)
        want, per = rig.want(nhyp, mask_words, key=key)
        assert_same(got, want, str(key))
        return got, per
    finally:
        rig.close()


@pytest.mark.parametrize("n", [0, 2, 3, 19, 20, 21, 63, 64, 65, 257])
def test_correspondence_counts_at_the_edges(afv, gpu_ctx, n):
    sc = S.world(100 + n, n=max(n, 8), s=0.5, outliers=0.2, noise=0.4)
    sc.mp2[n:] = -1                                                                   # the tiny N: eight features, N matches
    nhyp = 24 if n > 65 else 65
    got, per = run(afv, gpu_ctx, [sc], 288, nhyp, words_for(n), ("edges", n))      # mask_words minimal (0 for N = 0)
    assert got["n"][0] == n
    if n >= 19:
        assert 3 < got["count"].max() < n and got["count"].min() < got["count"].max()


@pytest.mark.parametrize("nhyp", [1, 63, 64, 65, 300])
def test_hypothesis_counts(afv, gpu_ctx, nhyp):
    sc = S.world(55, n=21, s=3.0, outliers=0.3, noise=0.3)
    full = cached(("nhyp", 300), lambda: sc.candidate(32, 300, 2))
    rig = Rig(afv, gpu_ctx, [sc], 32)
    try:
        code, got = rig.call(nhyp, 2)                                                 # one word more than the 21 correspondences need
        assert code == 0
        want = {k: np.asarray(full[k])[None] for k in KEYS}
        for k in ("count", "degenerate", "sim3", "inliers"):
            want[k] = want[k][:, :nhyp]                                                # hypothesis h depends on (seed, h) alone
        assert_same(got, want, "nhyp %d" % nhyp)
        assert not got["inliers"][..., 1].any()                                       # the unused word is written, and zero
    finally:
        rig.close()


@pytest.mark.parametrize("nc", [1, 7, 64])
def test_batches_against_their_candidates_one_by_one(afv, gpu_ctx, nc):
    scenes = [S.world(300 + c, n=12 + c % 9, s=(1.0, 0.5, 3.0)[c % 3], outliers=0.2, noise=0.3, fix_scale=c % 4 == 3) for c in range(nc)]
    rig = Rig(afv, gpu_ctx, scenes, 32)
    try:
        code, got = rig.call(16, 1)
        assert code == 0
        want, _ = rig.want(16, 1, key="batch")
        assert_same(got, want, "batch of %d" % nc)
        for c in range(nc):
            code, one = rig.call(16, 1, which=[c])
            assert code == 0
            assert_same(one, {k: got[k][c:c + 1] for k in KEYS}, "candidate %d alone" % c)
    finally:
        rig.close()


@pytest.mark.parametrize("n1", [255, 256, 257, 513])
def test_gather_workgroup_edges(afv, gpu_ctx, n1):
    sc = S.world(400 + n1, n=n1, outliers=0.1)
    rng = np.random.default_rng(n1)
    drop = rng.random(n1) < 0.6
    drop[[0, 63, 64, 254, n1 - 1]] = False                                            # the first and last lanes of wavefronts and workgroups stay
    sc.mp2[drop] = -1
    sc.idx1 = np.arange(n1, dtype=np.int32)
    sc.idx1[rng.permutation(n1)[:7]] = -1
    got, per = run(afv, gpu_ctx, [sc], 544, 6, words_for(n1), ("gather", n1))         # mask_words from the host-countable entries
    assert 60 < got["n"][0] < 0.55 * n1 and (np.diff(got["index1"][0, :got["n"][0]]) > 0).all()


@pytest.mark.parametrize("kind", [dict(desc_bytes=32), dict(desc_bytes=61), dict(float_dim=128)])
def test_table_and_store_kinds_give_the_same_answer(afv, gpu_ctx, kind):
    sc = S.world(61, n=33, s=0.5, outliers=0.25, noise=0.5)
    run(afv, gpu_ctx, [sc, S.skip_reasons()], 48, 20, 2, "kinds", **kind)


def scene_list():
    return [S.skip_reasons(), S.q1_bound(False), S.q1_bound(True), S.coincident(False), S.coincident(True), S.collinear(), S.z_zero(False),
            S.z_zero(True), S.counted(6), S.counted(7), S.world(9, n=6, levels=False), S.world(9, n=5, levels=False)]


def test_constructed_scenes_and_the_python_class(afv, gpu_ctx):
    scenes = scene_list()
    nhyp = 40
    got, per = run(afv, gpu_ctx, scenes, 32, nhyp, 1, "constructed")
    assert got["degenerate"][3].all() and not got["degenerate"][4].any() and not got["degenerate"][5].any()
    for c, sc in enumerate(scenes):
        for settings in ((0.99, 6, nhyp), (0.99, 3, 7), (0.5, 6, nhyp)):
            mine = afv.Sim3Solver(got["n"][c], got["index1"][c], got["count"][c], got["degenerate"][c], got["sim3"][c], got["inliers"][c], sc.n1)
            ref = sc.solver(per[c], nhyp)
            assert (mine.mRansacMaxIts, mine.mRansacMinInliers) == (ref.mRansacMaxIts, ref.mRansacMinInliers)   # the constructor's defaults
            mine.SetRansacParameters(*settings)
            ref.SetRansacParameters(*settings)
            assert mine.mRansacMaxIts == ref.mRansacMaxIts
            for step in range(12):                                                    # LoopClosing's iterate(5) until bNoMore
                a, b = mine.iterate(5), ref.iterate(5)
                assert (a[0] is None) == (b[0] is None) and a[1] == b[1] and a[3] == b[3] and np.array_equal(a[2], b[2]), (c, settings, step)
                if a[0] is not None:
                    assert raw(a[0]).tobytes() == raw(b[0]).tobytes()
                    assert raw(mine.GetEstimatedRotation()).tobytes() == raw(ref.sim3[ref.best][:9]).tobytes()
                    assert raw(mine.GetEstimatedTranslation()).tobytes() == raw(ref.sim3[ref.best][9:12]).tobytes()
                    assert np.float32(mine.GetEstimatedScale()) == ref.sim3[ref.best][12]
                assert (mine.mnIterations, mine.mnBestInliers, mine.best) == (ref.mnIterations, ref.mnBestInliers, ref.best)
                if a[1]:
                    break
            mine.SetRansacParameters(*settings)
            ref.SetRansacParameters(*settings)
            a, b = mine.find(), ref.find()
            assert (a[0] is None) == (b[0] is None) and a[2] == b[2] and np.array_equal(a[1], b[1])
        with pytest.raises(ValueError):
            mine.SetRansacParameters(0.99, 6, nhyp + 1)
        with pytest.raises(ValueError):
            mine.SetRansacParameters(0.99, 2, nhyp)


def test_batch_of_the_python_class(afv, gpu_ctx):
    """Sim3Solver.batch: one current keyframe, three candidates, through the public interface"""
    cands = [S.world(70, n=30, s=0.5, outliers=o, noise=0.3) for o in (0.2, 0.5, 0.8)]   # one seed: the same keyframe 1 and map 1
    base = cands[0]
    for sc in cands:
        assert np.array_equal(sc.cam1.Rcw, base.cam1.Rcw) and np.array_equal(sc.pos[:30], base.pos[:30])
        sc.sigma2_1 = base.sigma2_1
    rig = Rig(afv, gpu_ctx, cands, 48)
    try:
        t = rig.table                                                                 # slot 0 is keyframe 1 as every candidate sees it
        cam = lambda c: dict(Rcw=c.Rcw, tcw=c.tcw, fx=c.fx, fy=c.fy, cx=c.cx, cy=c.cy)
        cams = {0: cam(base.cam1), 1: cam(cands[0].cam2), 3: cam(cands[1].cam2), 5: cam(cands[2].cam2)}
        mp1, mp2, _, idx2 = rig.rows()
        seeds = [sc.seed for sc in cands]
        solvers = afv.Sim3Solver.batch(t, rig.points, 0, [1, 3, 5], mp1[:, :30], mp2[:, :30], idx2[:, :30], cams, False, seed=seeds, nhyp=32)
        assert len(solvers) == 3
        for c, (sol, sc) in enumerate(zip(solvers, cands)):
            ref_out = sc.candidate(32, 32, 1)
            ref = sc.solver(ref_out, 32)
            assert sol.N == ref.N and sol.mN1 == 30 and np.array_equal(sol.count, ref_out["count"])
            assert raw(sol.sim3).tobytes() == raw(ref_out["sim3"]).tobytes()
            sol.SetRansacParameters(0.99, 15, 32)
            ref.SetRansacParameters(0.99, 15, 32)
            a, b = sol.find(), ref.find()
            assert (a[0] is None) == (b[0] is None) and a[2] == b[2] and np.array_equal(a[1], b[1])
            if a[0] is not None:
                assert raw(a[0]).tobytes() == raw(b[0]).tobytes()
    finally:
        rig.close()


def test_a_cloned_table_answers_as_its_source(afv, gpu_ctx):
    sc = S.world(61, n=33, s=0.5, outliers=0.25, noise=0.5)
    rig = Rig(afv, gpu_ctx, [sc, S.skip_reasons()], 48)
    dst = afv.table.DescriptorTable(gpu_ctx, 4, 48)
    try:
        rig.table.clone_into(dst)
        code, got = rig.call(20, 2, table=dst)
        assert code == 0
        assert_same(got, rig.want(20, 2, key="kinds")[0], "clone")
    finally:
        dst.close()
        rig.close()


def test_a_slot_filled_from_a_frame(afv, gpu_ctx):
    """keyframe 1 arrives through afv_table_set_from_frame: its sigma2 plane is the frame's keyPtsSigma2 = size * size"""
    sc = S.world(62, n=25, s=3.0, outliers=0.2, noise=0.4)
    size = (np.float32(1.2) ** np.random.default_rng(1).integers(0, 8, sc.n1)).astype(np.float32) * np.float32(31.0)
    sc.sigma2_1 = size * size
    rig = Rig(afv, gpu_ctx, [sc], 32)
    fr = afv.Frame(gpu_ctx, max_x=640.0, max_y=480.0, cap=32)
    try:
        rng = np.random.default_rng(2)
        kps = np.zeros(sc.n1, afv.KP_DTYPE)
        kps["x"], kps["y"] = rng.uniform(20, 600, sc.n1), rng.uniform(20, 400, sc.n1)
        fr.set_features(kps, rng.integers(0, 256, (sc.n1, 32), dtype=np.uint8), sizes=size)
        rig.table.set_from_frame(0, fr)
        code, got = rig.call(20, 1)
        assert code == 0
        assert_same(got, rig.want(20, 1)[0], "from frame")
        assert got["max_err"][0, :sc.n1, 0].max() > 9 * 31 * 31
    finally:
        fr.close()
        rig.close()


def test_error_answers_leave_the_outputs_untouched(afv, gpu_ctx):
    L = afv._lib
    sc = S.world(61, n=33, s=0.5, outliers=0.25, noise=0.5)
    rig = Rig(afv, gpu_ctx, [sc, S.skip_reasons()], 48)
    other_ctx = afv.Context(max_width=640, max_height=480, max_batch=1)
    foreign = afv.MapPoints(other_ctx, 16)
    try:
        mp1, mp2, idx1, idx2 = rig.rows()
        pristine = rig.outputs(2, 20, 2)

        def refused(**over):
            out = rig.outputs(2, 20, 2)
            code, out = rig.call(over.pop("nhyp", 20), over.pop("mask_words", 2), out=out, **over)
            for k in KEYS:
                assert raw(out[k]).tobytes() == raw(pristine[k]).tobytes(), (over.keys(), k)
            return code

        def changed(a, r, i, v):
            b = a.copy()
            b[r, i] = v
            return b
        assert refused(nc=0) == L.EINVAL and refused(nc=65) == L.EINVAL
        assert refused(nhyp=0) == L.EINVAL and refused(nhyp=1025) == L.EINVAL
        assert refused(mask_words=-1) == L.EINVAL and refused(mask_words=257) == L.EINVAL
        assert refused(mask_words=1) == L.EINVAL                                       # 33 host-countable entries need two words
        bad_jobs = rig.jobs()
        bad_jobs[1].struct_size = 12
        assert refused(jobs=bad_jobs) == L.EINVAL
        bad_jobs = rig.jobs()
        bad_jobs[0].struct_size = bad_jobs[1].struct_size = 4
        assert refused(jobs=bad_jobs) == L.EINVAL
        bad_jobs = rig.jobs()
        bad_jobs[1].fix_scale = 2
        assert refused(jobs=bad_jobs) == L.EINVAL
        assert refused(slot_a=np.array([0, 4], np.int32)) == L.EINVAL and refused(slot_b=np.array([-1, 3], np.int32)) == L.EINVAL
        cap_p = rig.points.capacity
        assert refused(mp1=changed(mp1, 1, 3, cap_p)) == L.EINVAL and refused(mp2=changed(mp2, 0, 5, -2)) == L.EINVAL
        assert refused(idx2=changed(idx2, 0, 2, sc.n2)) == L.EINVAL and refused(idx2=changed(idx2, 1, 2, -2)) == L.EINVAL
        assert refused(idx1=changed(idx1, 0, 2, sc.n1)) == L.EINVAL
        assert refused(points=foreign) == L.EINVAL                                    # a store of another context
        for k in ("slot_a", "slot_b", "jobs", "mp1", "mp2", "idx2"):
            assert refused(**{k: None}) == L.EINVAL, k
        for k in KEYS[:6]:                                                            # a required output missing: the others stay untouched
            out = rig.outputs(2, 20, 2)
            keep = out[k]
            out[k] = None
            code, out = rig.call(20, 2, out=out)
            assert code == L.EINVAL, k
            out[k] = keep
            assert all(raw(out[q]).tobytes() == raw(pristine[q]).tobytes() for q in KEYS)
        rig.table.set(1, np.zeros((sc.n2, 32), np.uint8))                               # a recycled slot holds features without geometry
        assert refused() == L.EINVAL
        rig.table.set_geometry(1, np.zeros(sc.n2), np.zeros(sc.n2), sc.sigma2_2)
        code, got = rig.call(20, 2)                                                   # ... and the call works again, the optional outputs absent
        assert code == 0
        assert_same(got, rig.want(20, 2, key="kinds")[0], "after the refusals")
        out = rig.outputs(2, 20, 2)
        for k in KEYS[6:]:
            out[k] = None
        code, out = rig.call(20, 2, out=out)
        assert code == 0 and all(raw(out[k]).tobytes() == raw(got[k]).tobytes() for k in KEYS[:6])
    finally:
        foreign.close()
        other_ctx.close()
        rig.close()
