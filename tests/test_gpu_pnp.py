"""-m gpu: afv_frame_pnp_hypotheses (PnPsolver's constructor, every EPnP RANSAC hypothesis and the Refine of every record) against the
restatement tests/_pnp_ref.py, BIT FOR BIT: n, min_inliers, index, count, degenerate, the float bits of pose, the inlier words, refined,
refined_count, refined_pose, refined_inliers and the optional max_err / p3dw, then the iterate(5) / find traces of the Python class against
the sequential loop of the restatement.  Shapes are the smallest at which the kernels can go wrong: N at the mask-word and wavefront
edges, refinements over 10 / 63 / 64 / 65 / 129 inliers, nhyp 1 / 63 / 64 / 65 / 300, batches against their candidates one by one, feature
counts on both sides of the gather workgroup (256), minimal and generous mask_words, frames of binary, 61-byte and float rows, every error
answer, the degenerate and coplanar scenes and the chain into PoseOptimizationBatch.  The sigma2 plane is read from the device
(Context.size_sigma), everything else comes from the scene."""
import functools

import numpy as np
import pytest

import _pnp_ref as R
import _pnp_scenes as S
import _poseopt_ref as PR

pytestmark = pytest.mark.gpu
KEYS = ("count", "degenerate", "pose", "inliers", "refined", "refined_count", "refined_pose", "refined_inliers", "index", "max_err", "p3dw")


def twc(Rcw, tcw):
    return np.array([-Rcw[0, k] * tcw[0] + (-Rcw[1, k] * tcw[1] + -Rcw[2, k] * tcw[2]) for k in range(3)], np.float32)


class Rig:
    """a scene on the device: the store and the frame with its features and intrinsics"""

    def __init__(self, afv, ctx, s, desc_bytes=32, float_dim=0, cap=None):
        self.afv, self.s = afv, s
        self.points = afv.MapPoints(ctx, len(s.store_flags))
        ids = np.flatnonzero(s.store_flags & R.SET)
        if len(ids):
            self.points.set(ids, pos=s.store_pos[ids])
        bad = np.flatnonzero(s.store_flags & R.BAD)
        if len(bad):
            self.points.set_flags(bad, bad=np.ones(len(bad), np.uint8))
        self.frame = afv.Frame(ctx, max_x=S.W, max_y=S.H, cap=max(s.N, 1) if cap is None else cap, desc_bytes=desc_bytes, float_dim=float_dim)
        kps = np.zeros(s.N, afv.KP_DTYPE)
        kps["x"], kps["y"], kps["octave"] = s.x, s.y, s.octave
        rows = np.zeros((s.N, float_dim), np.float32) if float_dim else np.zeros((s.N, desc_bytes), np.uint8)
        self.frame.set_features(kps, rows)
        Rc, tc = s.Rcw.astype(np.float32), s.tcw.astype(np.float32)
        self.frame.set_pose(Rc, tc, twc(Rc, tc), *s.cam)
        self.sigma2 = ctx.size_sigma(kps)[1]

    def call(self, nhyp=None, mask_words=None, rows=None, seeds=None):
        s = self.s
        rows = s.rows if rows is None else rows
        seeds = [s.seed + c for c in range(len(rows))] if seeds is None else seeds
        jobs = self.afv.pnp.pnp_jobs(seeds, s.min_inliers, s.epsilon, s.th2)
        return self.afv.pnp.hypotheses(self.frame, self.points, jobs, rows, s.nhyp if nhyp is None else nhyp, mask_words, extras=True)

    def close(self):
        self.frame.close()
        self.points.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_candidate(got, c, want, tag):
    assert int(got["n"][c]) == want["n"] and int(got["min_inliers"][c]) == want["min_inliers"], (tag, got["n"][c], want["n"], got["min_inliers"][c])
    for k in KEYS:
        assert same_bits(got[k][c], want[k]), (tag, k, np.argwhere(np.asarray(got[k][c]) != np.asarray(want[k]))[:4], got[k][c].ravel()[:12],
                                               want[k].ravel()[:12])


def check_scene(afv, ctx, s, nhyp=None, mask_words=None, **rig):
    r = Rig(afv, ctx, s, **rig)
    try:
        got = r.call(nhyp, mask_words)
        wants = [s.run(c, r.sigma2, nhyp, mask_words) for c in range(s.nc)]
        for c in range(s.nc):
            assert_candidate(got, c, wants[c], (s.name, c))
        return got, wants, r.sigma2
    finally:
        r.close()


@pytest.mark.parametrize("n", (4, 5, 31, 32, 33, 63, 64, 65, 129, 300))
def test_correspondence_counts(afv, gpu_ctx, n):
    """N at the mask-word and wavefront edges; every feature matched, a fifth of them outliers, octaves mixed"""
    s = S.build("n%d" % n, n, n, n // 5, 100 + n, octaves=True, min_inliers=4, epsilon=0.3, nhyp=8)
    got, wants, _ = check_scene(afv, gpu_ctx, s)
    assert wants[0]["n"] == n and (n < 20 or wants[0]["refined"].any())


@pytest.mark.parametrize("n_in", (10, 63, 64, 65, 129))
def test_refinement_sizes(afv, gpu_ctx, n_in):
    """a record of exactly n_in inliers is refined: n_in clean matches + 7 outliers"""
    s = S.build("refine%d" % n_in, n_in + 12, n_in + 7, 7, 200 + n_in, min_inliers=10, epsilon=0.1, nhyp=12, seed=5 if n_in == 10 else 1)
    got, wants, _ = check_scene(afv, gpu_ctx, s)
    rec = np.flatnonzero(wants[0]["refined"] == 1)
    assert len(rec) and n_in in wants[0]["count"][rec], wants[0]["count"]


@pytest.mark.parametrize("nhyp", (1, 63, 64, 65, 300))
def test_hypothesis_counts(afv, gpu_ctx, nhyp):
    s = S.build("nhyp", 40, 36, 12, 7, bad=2, unset=2, min_inliers=10, epsilon=0.5)
    check_scene(afv, gpu_ctx, s, nhyp=nhyp)


@functools.lru_cache(None)
def batch_scene():
    return S.build("batch", 70, 50, 10, 11, nc=64, false_rows=tuple(range(1, 64, 3)), bad=3, unset=3, octaves=True, min_inliers=10, epsilon=0.4, nhyp=4)


@pytest.mark.parametrize("nc", (1, 7, 64))
def test_batches_equal_single_calls(afv, gpu_ctx, nc):
    s = batch_scene()
    r = Rig(afv, gpu_ctx, s)
    try:
        got = r.call(rows=s.rows[:nc])
        for c in range(nc):
            assert_candidate(got, c, s.run(c, r.sigma2), ("batch", nc, c))
            if nc == 7:
                one = r.call(rows=s.rows[c:c + 1], seeds=[s.seed + c])
                for k in KEYS + ("n", "min_inliers"):
                    assert same_bits(one[k][0], got[k][c]), (nc, c, k)
    finally:
        r.close()


@pytest.mark.parametrize("n", (255, 256, 257, 513))
def test_gather_workgroup_edges(afv, gpu_ctx, n):
    """feature counts on both sides of the gather workgroup's 256 lanes; a third of the features unmatched, bad and never-set ids.
    513 features is above the 300 the other frames stay within: it is the smallest count at which the gather loop runs a third chunk
    behind two full ones (the running base is carried twice); three hypotheses keep it cheap"""
    s = S.build("gather%d" % n, n, (2 * n) // 3, n // 6, 300 + n, bad=9, unset=9, octaves=True, nhyp=3)
    got, wants, _ = check_scene(afv, gpu_ctx, s)
    assert wants[0]["n"] == (2 * n) // 3


@pytest.mark.parametrize("mask_words", ("minimal", 256))
def test_mask_words(afv, gpu_ctx, mask_words):
    s = S.build("words", 70, 40, 8, 21, nhyp=6)   # 40 ids >= 0: two words at least
    check_scene(afv, gpu_ctx, s, mask_words=2 if mask_words == "minimal" else mask_words)


@pytest.mark.parametrize("kind", ("binary32", "binary61", "float64"))
def test_descriptor_kinds(afv, gpu_ctx, kind):
    """descriptors are not read: frames of every row kind answer the same"""
    s = S.build("rows", 50, 40, 8, 31, nhyp=6)
    check_scene(afv, gpu_ctx, s, **dict(binary32={}, binary61=dict(desc_bytes=61), float64=dict(float_dim=64))[kind])


def test_frame_capacity_above_its_features(afv, gpu_ctx):
    s = S.build("cap", 50, 40, 8, 41, nhyp=6)
    check_scene(afv, gpu_ctx, s, cap=300)


@pytest.mark.parametrize("name", ("identical", "coplanar", "too_few", "below_four"))
def test_degenerate_scenes(afv, gpu_ctx, name):
    s = dict(identical=lambda: S.build("identical", 6, 6, 0, 51, identical=True, min_inliers=4, nhyp=6),
             coplanar=lambda: S.build("coplanar", 30, 30, 5, 52, planar=True, min_inliers=10, nhyp=20),
             too_few=lambda: S.build("too_few", 20, 8, 0, 53, min_inliers=10, nhyp=6),
             below_four=lambda: S.build("below_four", 20, 3, 0, 54, min_inliers=4, nhyp=6))[name]()
    got, wants, _ = check_scene(afv, gpu_ctx, s)
    if name == "identical":
        assert wants[0]["degenerate"].all() and not wants[0]["count"].any()
    if name == "below_four":
        assert wants[0]["n"] == 3 and not wants[0]["degenerate"].any() and not wants[0]["count"].any()


def test_solver_traces(afv, gpu_ctx):
    """PnPsolver.batch: iterate(5) until bNoMore or an answer, and find, against the sequential loop of the restatement"""
    s = S.build("trace", 60, 45, 15, 61, nc=4, false_rows=(1, 3), bad=2, unset=2, min_inliers=10, epsilon=0.5, nhyp=35)
    r = Rig(afv, gpu_ctx, s)
    try:
        for mode in ("iterate", "find"):
            solvers = afv.PnPsolver.batch(r.frame, r.points, s.rows, seed=s.seed, nhyp=s.nhyp, minInliers=s.min_inliers, epsilon=s.epsilon, th2=s.th2)
            assert len(solvers) == s.nc
            for c, dev in enumerate(solvers):
                ref = s.solver(c, r.sigma2)
                assert dev.mRansacMaxIts == ref.mRansacMaxIts and dev.mRansacMinInliers == ref.mRansacMinInliers
                for _ in range(40):
                    if mode == "iterate":
                        a, b = dev.iterate(5), ref.iterate(5)
                    else:
                        fa, fb = dev.find(), ref.find()
                        a, b = (fa[0], True, fa[1], fa[2]), (fb[0], True, fb[1], fb[2])
                    assert (a[0] is None) == (b[0] is None) and a[1] == b[1] and a[3] == b[3] and np.array_equal(a[2], b[2]), (mode, c)
                    assert a[0] is None or same_bits(a[0], b[0]), (mode, c)
                    assert dev.mnIterations == ref.mnIterations
                    if a[1] or a[0] is not None or mode == "find":
                        break
        T, _, vb, n = afv.PnPsolver.batch(r.frame, r.points, s.rows[:1], seed=s.seed, nhyp=s.nhyp)[0].iterate(5)
        assert T is not None and n > s.min_inliers and vb.sum() == n
    finally:
        r.close()


def test_chain_into_pose_optimization(afv, gpu_ctx):
    """Relocalization (Tracking.cc:1218-1245): the pose of a successful iterate is the initial pose, its inliers the pts of a pose job"""
    s = S.build("chain", 80, 60, 15, 71, min_inliers=10, epsilon=0.5, nhyp=35)
    r = Rig(afv, gpu_ctx, s)
    try:
        sol = r.frame.PnPsolverBatch(r.points, s.rows, seed=s.seed, nhyp=s.nhyp)[0]
        T, no_more, vb, n = sol.iterate(5)
        ref = s.solver(0, r.sigma2)
        Tr, _, vbr, nr = ref.iterate(5)
        assert T is not None and same_bits(T, Tr) and np.array_equal(vb, vbr) and n == nr
        pts = np.where(vb, s.rows[0], -1).astype(np.int32)
        got = r.frame.PoseOptimizationBatch(r.points, [(pts, T[:3, :3], T[:3, 3])])[0]
        kps = np.zeros(s.N, afv.KP_DTYPE)
        kps["x"], kps["y"], kps["octave"] = s.x, s.y, s.octave
        inf = gpu_ctx.size_sigma(kps)[2]
        prob = PR.Problem(s.x, s.y, np.full(s.N, -1, np.float32), inf, pts, s.store_pos, (s.store_flags & R.SET) != 0, *s.cam, 0.0)
        want = PR.pose_optimization(prob, np.ascontiguousarray(T[:3, :3]), np.ascontiguousarray(T[:3, 3]))
        assert same_bits(got["Rcw"].reshape(9), want.Rcw) and same_bits(got["tcw"], want.tcw) and got["n_good"] == want.n_good
        assert np.array_equal(got["outlier"], want.outlier != 0) and got["n_good"] >= 40
    finally:
        r.close()


def test_error_answers_leave_the_outputs_untouched(afv, gpu_ctx):
    s = S.build("errors", 40, 30, 5, 81, nhyp=4)
    r = Rig(afv, gpu_ctx, s)
    L = afv._lib
    lib = L.load()
    try:
        def call(frame=r.frame, points=r.points, rows=s.rows, nc=1, nhyp=4, mask_words=2, min_inliers=10, epsilon=0.5, th2=5.991, size=None,
                 null=None):
            jobs = afv.pnp.pnp_jobs([1] * max(nc, 1), min_inliers, epsilon, th2)
            if size is not None:
                jobs[0].struct_size = size
            rows = np.ascontiguousarray(rows, np.int32)
            h, w = (nhyp, mask_words) if 1 <= nhyp <= 1024 and 0 <= mask_words <= 256 else (1, 1)
            m = max(nc, 1)
            outs = [np.full(m, 7, np.int32), np.full(m, 7, np.int32), np.full((m, s.N), 7, np.int32), np.full((m, h), 7, np.int32),
                    np.full((m, h), 7, np.uint8), np.full((m, h, 12), 7, np.float32), np.full((m, h, max(w, 1)), 7, np.uint32),
                    np.full((m, h), 7, np.uint8), np.full((m, h), 7, np.int32), np.full((m, h, 12), 7, np.float32),
                    np.full((m, h, max(w, 1)), 7, np.uint32), np.full((m, s.N), 7, np.float32), np.full((m, s.N, 3), 7, np.float32)]
            args = [frame.handle if frame is not None else None, points.handle if points is not None else None, jobs, nc, L.ptr(rows), nhyp,
                    mask_words] + [L.ptr(o) for o in outs]
            if null is not None:
                args[null] = None
            rc = lib.afv_frame_pnp_hypotheses(*args)
            assert all((o == 7).all() for o in outs), "outputs were written"
            return rc
        bad = s.rows.copy()
        bad[0, 0] = len(s.store_flags)
        below = s.rows.copy()
        below[0, 0] = -2
        empty = afv.Frame(gpu_ctx, max_x=S.W, max_y=S.H, cap=8)
        poseless = afv.Frame(gpu_ctx, max_x=S.W, max_y=S.H, cap=s.N)
        kps = np.zeros(s.N, afv.KP_DTYPE)
        kps["x"], kps["y"] = s.x, s.y
        poseless.set_features(kps, np.zeros((s.N, 32), np.uint8))
        other = afv.Context(max_width=640, max_height=480, max_batch=1)
        foreign = afv.MapPoints(other, len(s.store_flags))
        cases = dict(null_frame=dict(null=0), null_points=dict(null=1), null_jobs=dict(null=2), null_pts=dict(null=4),
                     nc0=dict(nc=0), nc65=dict(nc=65), nhyp0=dict(nhyp=0), nhyp1025=dict(nhyp=1025), words_neg=dict(mask_words=-1),
                     words257=dict(mask_words=257), words_short=dict(mask_words=0), id_above=dict(rows=bad), id_below=dict(rows=below),
                     size0=dict(size=0), size_odd=dict(size=23), min3=dict(min_inliers=3), eps0=dict(epsilon=0.0), eps_nan=dict(epsilon=float("nan")),
                     eps_inf=dict(epsilon=float("inf")), th0=dict(th2=0.0), th_neg=dict(th2=-1.0), th_nan=dict(th2=float("nan")),
                     no_features=dict(frame=empty), no_pose=dict(frame=poseless), foreign_store=dict(points=foreign))
        cases.update({"null_out%d" % k: dict(null=k) for k in range(7, 18)})
        for name, kw in cases.items():
            assert call(**kw) in (L.EINVAL, L.EUNSUPPORTED), name
        for o in (empty, poseless, foreign):
            o.close()
        other.close()
        with pytest.raises(Exception):
            r.call(mask_words=0)
    finally:
        r.close()
