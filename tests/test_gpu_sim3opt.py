"""-m gpu: afv_table_optimize_sim3 (csrc/k_sim3opt.hip) against the restatement (tests/_sim3opt_ref.py), bit for bit: the Sim3 doubles,
the counts, the per-feature states and the trace of both optimize() calls.  Every constructed scene; correspondence counts at the
minimum-correspondence rule and at the edges of the 64 strided partial sums; a slot filled to cap; batches against their jobs one by one
with slots of unequal size; the three table kinds; a cloned table and a slot promoted from a frame (both must bring the information
plane); every error answer with the outputs untouched; the chain Sim3Solver.batch -> find -> OptimizeSim3.  Nothing here provokes a
fault: every scene uses finite inputs that the restatement handles by rule."""
import ctypes as C

import numpy as np
import pytest

import _sim3_ref as R3
import _sim3opt_ref as R
import _sim3opt_scenes as S

pytestmark = pytest.mark.gpu
_cache = {}


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def want_of(key, sc):
    return cached(key, sc.solve)


class Rig:
    """scenes installed in a table (scene c: slots 2c and 2c + 1) and a store (scene c: ids from base[c] on)"""

    def __init__(self, afv, ctx, scenes, cap, desc_bytes=32, float_dim=0, spare=3, inf=True):
        self.afv, self.ctx, self.scenes, self.cap = afv, ctx, scenes, cap
        kind = {"float_dim": float_dim} if float_dim else {"desc_bytes": desc_bytes}
        self.table = afv.table.DescriptorTable(ctx, 2 * len(scenes), cap, **kind)
        self.base = np.cumsum([0] + [len(sc.pos) for sc in scenes])
        self.points = afv.MapPoints(ctx, int(self.base[-1]) + spare, **kind)
        rng = np.random.default_rng(4)
        for c, sc in enumerate(scenes):
            for slot, n, x, y, f in ((2 * c, sc.n1, sc.x1, sc.y1, sc.inf1), (2 * c + 1, sc.n2, sc.x2, sc.y2, sc.inf2)):
                rows = rng.normal(0, 1, (n, float_dim)).astype(np.float32) if float_dim else rng.integers(0, 256, (n, desc_bytes), dtype=np.uint8)
                self.table.set(slot, rows)
                self.table.set_geometry(slot, x, y, np.ones(n, np.float32))
                if inf:
                    self.table.set_inf(slot, f)
            ids = np.nonzero(sc.flags & R3.SET)[0].astype(np.int32)
            if len(ids):
                self.points.set(ids + self.base[c], pos=sc.pos[ids])
                self.points.set_flags(ids + self.base[c], bad=(sc.flags[ids] & R3.BAD) != 0)

    def close(self):
        self.points.close()
        self.table.close()

    def rows(self, sel):
        out = {k: np.full((len(sel), self.cap), -1, np.int32) for k in ("mp1", "mp2", "idx2")}
        for r, c in enumerate(sel):
            sc = self.scenes[c]
            for k in ("mp1", "mp2"):
                v = getattr(sc, k)
                out[k][r, :sc.n1] = np.where(v >= 0, v + self.base[c], -1)
            out["idx2"][r, :sc.n1] = sc.idx2
        return out["mp1"], out["mp2"], out["idx2"]

    def jobs(self, sel):
        L = self.afv._lib
        jobs = (L.Sim3OptJob * len(sel))()
        for r, c in enumerate(sel):
            sc, j = self.scenes[c], jobs[r]
            j.struct_size, j.fix_scale, j.th2 = C.sizeof(L.Sim3OptJob), int(sc.fix_scale), float(sc.th2)
            for side, cam in (("1", sc.cam1), ("2", sc.cam2)):
                for k in range(9):
                    getattr(j, "Rcw" + side)[k] = float(cam.Rcw[k])
                for k in range(3):
                    getattr(j, "tcw" + side)[k] = float(cam.tcw[k])
                for key in ("fx", "fy", "cx", "cy"):
                    setattr(j, key + side, float(getattr(cam, key)))
            for k in range(9):
                j.R12[k] = float(sc.R12[k])
            for k in range(3):
                j.t12[k] = float(sc.t12[k])
            j.s12 = float(sc.s12)
        return jobs

    def outputs(self, nc, poison=0xA5):
        L = self.afv._lib
        res = (L.Sim3OptResult * nc)()
        C.memset(res, poison, C.sizeof(res))
        return res, np.full((nc, self.cap), poison, np.uint8)

    def call(self, which=None, table=None, points=None, out=None, **over):
        """the C entry point as it is: returns (code, results, state).  Outputs start poisoned: what the call leaves is what it wrote"""
        sel = list(range(len(self.scenes))) if which is None else list(which)
        nc = len(sel)
        mp1, mp2, idx2 = self.rows(sel)
        a = dict(slot_a=np.array([2 * c for c in sel], np.int32), slot_b=np.array([2 * c + 1 for c in sel], np.int32), jobs=self.jobs(sel), nc=nc,
                 mp1=mp1, mp2=mp2, idx2=idx2)
        a.update(over)
        res, state = out or self.outputs(nc)
        a.setdefault("results", res)
        a.setdefault("state", state)
        p = self.afv._lib.ptr
        code = self.table.lib.afv_table_optimize_sim3((table or self.table).handle, (points or self.points).handle, p(a["slot_a"]), p(a["slot_b"]),
                                                      a["jobs"], a["nc"], p(a["mp1"]), p(a["mp2"]), p(a["idx2"]), a["results"], p(a["state"]))
        return code, res, state


def res_bytes(r):
    return bytes(memoryview(r).cast("B")) if not isinstance(r, bytes) else r


def one(res, c):
    return C.string_at(C.addressof(res[c]), C.sizeof(res[c]))


def assert_job(res, state, c, sc, w, name):
    """result c and state row c against a restatement Result, bit for bit"""
    g = res[c]
    ints = (g.n_in, g.n_corr, g.n_bad, g.more_iterations, g.early, g.iterations[0], g.iterations[1], g.trials[0], g.trials[1], g.reserved)
    want = (w.n_in, w.n_corr, w.n_bad, w.more_iterations, w.early, int(w.iterations[0]), int(w.iterations[1]), int(w.trials[0]), int(w.trials[1]), 0)
    assert ints == want, (name, c, ints, want)
    got = np.array(list(g.R12) + list(g.t12) + [g.s12] + list(g.chi2) + list(g.lam), np.float64)
    ref = np.concatenate([w.R12, w.t12, [w.s12], w.chi2, w.lam]).astype(np.float64)
    assert got.tobytes() == ref.tobytes(), (name, c, got, ref)
    assert np.array_equal(state[c, :sc.n1], w.state), (name, c)
    assert not state[c, sc.n1:].any(), (name, c)


def run(afv, ctx, named, cap, **kind):
    """named: [(key, scene)]: one call over all of them, every job against the restatement"""
    rig = Rig(afv, ctx, [sc for _, sc in named], cap, **kind)
    try:
        code, res, state = rig.call()
        assert code == 0, afv._lib.strerror(code)
        for c, (key, sc) in enumerate(named):
            assert_job(res, state, c, sc, want_of(key, sc), key)
        return res, state
    finally:
        rig.close()


def test_every_constructed_scene(afv, gpu_ctx):
    named = sorted(S.every_scene().items())
    res, state = run(afv, gpu_ctx, named, 48)
    by = {k: res[c] for c, (k, _) in enumerate(named)}
    assert by["clean"].more_iterations == 5 and by["planted_outliers"].more_iterations == 10
    assert by["survivors_10"].early == 0 and by["survivors_9"].early == 1 and by["no_edges"].n_corr == 0
    assert (state == afv._lib.SIM3OPT_REMOVED_SECOND).any() and (state == afv._lib.SIM3OPT_NOT_EDGE).any()


@pytest.mark.parametrize("n", [9, 10, 11, 63, 64, 65, 128, 300])
def test_correspondence_counts_at_the_edges(afv, gpu_ctx, n):
    sc = S.sized(n)
    res, _ = run(afv, gpu_ctx, [(("sized", n), sc)], 320)
    assert res[0].n_corr == n and (n < 10 or res[0].iterations[1] > 0 or res[0].early)


def test_a_slot_filled_to_cap(afv, gpu_ctx):
    sc = S.sized(70, seed=71)
    assert sc.n1 == 70 and sc.n2 == 75
    run(afv, gpu_ctx, [("cap b", sc)], 75)                              # keyframe 2 fills its slot
    sc = S.world(72, n=64, s=0.5, outliers=0.1, noise=0.4, extra2=0)
    assert sc.n1 == sc.n2 == 64
    run(afv, gpu_ctx, [("cap both", sc)], 64)                           # both keyframes fill theirs: no row behind n1


@pytest.mark.parametrize("nc", [1, 7, 64])
def test_batches_against_their_jobs_one_by_one(afv, gpu_ctx, nc):
    named = [(("batch", c), S.world(300 + c, n=12 + 5 * (c % 9), s=(1.0, 0.5, 3.0)[c % 3], outliers=(0.0, 0.2)[c % 2], noise=0.3, fix_scale=c % 4 == 3))
             for c in range(nc)]
    rig = Rig(afv, gpu_ctx, [sc for _, sc in named], 64)
    try:
        code, res, state = rig.call()
        assert code == 0
        for c, (key, sc) in enumerate(named):
            assert_job(res, state, c, sc, want_of(key, sc), key)
        for c in range(0, nc, max(1, nc // 8)):                         # ... and alone: the same bytes
            code, r1, s1 = rig.call(which=[c])
            assert code == 0
            assert one(r1, 0) == one(res, c) and np.array_equal(s1[0], state[c]), c
    finally:
        rig.close()


@pytest.mark.parametrize("kind", [dict(desc_bytes=32), dict(desc_bytes=61), dict(float_dim=128)])
def test_table_and_store_kinds_give_the_same_answer(afv, gpu_ctx, kind):
    run(afv, gpu_ctx, [("planted_outliers", S.planted_outliers()), ("filter_clauses", S.filter_clauses())], 48, **kind)


def test_a_cloned_table_brings_the_information_plane(afv, gpu_ctx):
    named = [("planted_outliers", S.planted_outliers()), ("filter_clauses", S.filter_clauses())]
    rig = Rig(afv, gpu_ctx, [sc for _, sc in named], 48)
    dst = afv.table.DescriptorTable(gpu_ctx, 4, 48)
    try:
        rig.table.clone_into(dst)
        code, res, state = rig.call(table=dst)
        assert code == 0
        for c, (key, sc) in enumerate(named):
            assert_job(res, state, c, sc, want_of(key, sc), "clone " + key)
        rig.table.set(1, np.zeros((named[0][1].n2, 32), np.uint8))       # afv_table_set forgets the plane ...
        rig.table.set_geometry(1, named[0][1].x2, named[0][1].y2, np.ones(named[0][1].n2))
        assert rig.call()[0] == afv._lib.EINVAL
        rig.table.clone_into(dst)                                        # ... and a clone carries that too
        assert rig.call(table=dst)[0] == afv._lib.EINVAL
    finally:
        dst.close()
        rig.close()


def test_a_slot_promoted_from_a_frame_brings_its_information(afv, gpu_ctx):
    """keyframe 1 arrives through afv_table_set_from_frame: its information plane is the frame's keyPtsInf = 1 / size^2"""
    sc = S.world(60, n=25, s=3.0, outliers=0.2, noise=0.4)
    assert 10 < sc.x1.min() and sc.x1.max() < 630 and 10 < sc.y1.min() and sc.y1.max() < 470   # every keypoint inside the frame's image
    size = (np.float32(1.2) ** np.random.default_rng(1).integers(0, 4, sc.n1)).astype(np.float32)
    sc.inf1 = (np.float32(1.0) / (size * size)).astype(np.float32)
    rig = Rig(afv, gpu_ctx, [sc], 32, inf=False)
    fr = afv.Frame(gpu_ctx, max_x=640.0, max_y=480.0, cap=32)
    try:
        rig.table.set_inf(1, sc.inf2)
        assert rig.call()[0] == afv._lib.EINVAL                         # slot 0 holds features without the plane
        kps = np.zeros(sc.n1, afv.KP_DTYPE)
        kps["x"], kps["y"] = sc.x1, sc.y1
        fr.set_features(kps, np.random.default_rng(2).integers(0, 256, (sc.n1, 32), dtype=np.uint8), sizes=size)
        rig.table.set_from_frame(0, fr)
        code, res, state = rig.call()
        assert code == 0
        assert_job(res, state, 0, sc, sc.solve(), "from frame")
    finally:
        fr.close()
        rig.close()


def test_error_answers_leave_the_outputs_untouched(afv, gpu_ctx):
    L = afv._lib
    named = [("planted_outliers", S.planted_outliers()), ("filter_clauses", S.filter_clauses())]
    sc = named[0][1]
    rig = Rig(afv, gpu_ctx, [s for _, s in named], 48)
    other_ctx = afv.Context(max_width=640, max_height=480, max_batch=1)
    foreign = afv.MapPoints(other_ctx, 16)
    try:
        mp1, mp2, idx2 = rig.rows([0, 1])
        p_res, p_state = rig.outputs(2)

        def refused(**over):
            out = rig.outputs(2)
            code, res, state = rig.call(out=out, **over)
            assert res_bytes(res) == res_bytes(p_res) and np.array_equal(state, p_state), over.keys()
            return code

        def changed(a, r, i, v):
            b = a.copy()
            b[r, i] = v
            return b
        assert refused(nc=0) == L.EINVAL and refused(nc=65) == L.EINVAL
        bad = rig.jobs([0, 1])
        bad[1].struct_size = 12
        assert refused(jobs=bad) == L.EINVAL
        bad = rig.jobs([0, 1])
        bad[0].struct_size = bad[1].struct_size = 4
        assert refused(jobs=bad) == L.EINVAL
        bad = rig.jobs([0, 1])
        bad[1].fix_scale = 2
        assert refused(jobs=bad) == L.EINVAL
        assert refused(slot_a=np.array([0, 4], np.int32)) == L.EINVAL and refused(slot_b=np.array([-1, 3], np.int32)) == L.EINVAL
        cap_p = rig.points.capacity
        assert refused(mp1=changed(mp1, 1, 3, cap_p)) == L.EINVAL and refused(mp2=changed(mp2, 0, 5, -2)) == L.EINVAL
        assert refused(idx2=changed(idx2, 0, 2, sc.n2)) == L.EINVAL and refused(idx2=changed(idx2, 1, 2, -2)) == L.EINVAL
        assert refused(points=foreign) == L.EINVAL                      # a store of another context
        for k in ("slot_a", "slot_b", "jobs", "mp1", "mp2", "idx2", "results", "state"):
            assert refused(**{k: None}) == L.EINVAL, k
        rig.table.set(1, np.zeros((sc.n2, 32), np.uint8))                 # a recycled slot: features without geometry, then without information
        assert refused() == L.EINVAL
        rig.table.set_geometry(1, sc.x2, sc.y2, np.ones(sc.n2))
        assert refused() == L.EINVAL
        assert b"information" in rig.table.lib.afv_last_error(rig.ctx.handle)
        rig.table.set_inf(1, sc.inf2)
        code, res, state = rig.call()                                     # ... and the call works again
        assert code == 0
        for c, (key, s) in enumerate(named):
            assert_job(res, state, c, s, want_of(key, s), "after the refusals")
    finally:
        foreign.close()
        other_ctx.close()
        rig.close()


def test_the_chain_solver_find_optimize(afv, gpu_ctx):
    """LoopClosing::ComputeSim3 on one candidate through the public interface: Sim3Solver.batch -> find -> OptimizeSim3 with the solver's
    inliers as vpMatches1 and its estimate as the start"""
    sc = S.world(70, n=40, s=0.5, outliers=0.2, noise=0.3)
    rig = Rig(afv, gpu_ctx, [sc], 48)
    try:
        cam = lambda c: dict(Rcw=c.Rcw, tcw=c.tcw, fx=c.fx, fy=c.fy, cx=c.cx, cy=c.cy)
        cams = {0: cam(sc.cam1), 1: cam(sc.cam2)}
        mp1, mp2, idx2 = (v[:, :sc.n1] for v in rig.rows([0]))
        sol = afv.Sim3Solver.batch(rig.table, rig.points, 0, [1], mp1, mp2, idx2, cams, False, seed=5, nhyp=64)[0]
        sol.SetRansacParameters(0.99, 20, 64)
        T, inl, n = sol.find()
        assert T is not None and n >= 20
        S12 = (sol.GetEstimatedRotation(), sol.GetEstimatedTranslation(), sol.GetEstimatedScale())
        matches = np.where(inl, mp2[0], -1).astype(np.int32)
        n_in, out, (R12, t12, s12) = afv.OptimizeSim3(rig.table, rig.points, 0, 1, mp1[0], matches, idx2[0], cams, S12, th2=10, fix_scale=False)
        ref = S.Scene.__new__(S.Scene)
        ref.__dict__.update(sc.__dict__)
        ref.mp2 = np.where(inl, sc.mp2, -1).astype(np.int32)
        ref.R12, ref.t12, ref.s12 = np.float32(S12[0]).reshape(9), np.float32(S12[1]), np.float32(S12[2])
        w = ref.solve()
        assert n_in == w.n_in >= 10 and not w.early
        assert np.array_equal(out, np.where(w.mp2_out >= 0, w.mp2_out + rig.base[0], -1))
        assert R12.tobytes() == w.R12.reshape(3, 3).tobytes() and t12.tobytes() == w.t12.tobytes() and np.float64(s12).tobytes() == np.float64(w.s12).tobytes()
        assert abs(s12 - 0.5) < 0.01
        three = afv.OptimizeSim3Batch(rig.table, rig.points, 0, [1, 1, 1], mp1[0], np.stack([matches] * 3), np.stack([idx2[0]] * 3), cams, [S12] * 3)
        assert all(b[0] == n_in and np.array_equal(b[1], out) and b[2][0].tobytes() == R12.tobytes() for b in three)
    finally:
        rig.close()
