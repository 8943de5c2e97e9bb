"""-m gpu: afv_frame_pose_optimize (Optimizer::PoseOptimization on a resident frame) against the restatement tests/_poseopt_ref.py, BIT FOR
BIT: the 12 pose floats, mvbOutlier, n_good, n_edges, rounds and the per-round trace (iterations, trials, chi2, lambda; a NaN equals a NaN) -
on every constructed scene of tests/_poseopt_scenes.py (tests/test_poseopt_ref_cpu.py proves that each reaches its rule), on seeded random
scenes at the wavefront, workgroup and features-per-thread edges, in batches, after a store update, in the chain with SearchLocalPoints,
and through the C++ adapter.  keyPtsInf is read from the device (Context.size_sigma), everything else comes from the scene."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _poseopt_ref as R
import _poseopt_scenes as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "anyfeature-vslam_amd", "adapter", "poseopt_selftest")
CONSTRUCTED = S.constructed()
SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2047, 8192)


def twc(Rcw, tcw):
    return np.array([-Rcw[0, k] * tcw[0] + (-Rcw[1, k] * tcw[1] + -Rcw[2, k] * tcw[2]) for k in range(3)], np.float32)


class Rig:
    """a scene on the device: the store, the frame with its features and the scene's initial pose"""

    def __init__(self, afv, ctx, s):
        self.afv, self.s = afv, s
        self.points = afv.MapPoints(ctx, len(s.store_set))
        ids = np.flatnonzero(s.store_set)
        if len(ids):
            self.points.set(ids, pos=s.store_pos[ids])
        self.frame = afv.Frame(ctx, max_x=S.W, max_y=S.H, cap=max(s.N, 1))
        kps = np.zeros(s.N, afv.KP_DTYPE)
        kps["x"], kps["y"], kps["octave"] = s.x, s.y, s.octave
        self.frame.set_features(kps, np.zeros((s.N, 32), np.uint8), u_right=s.u_right)
        self.frame.set_pose(s.Rcw, s.tcw, twc(s.Rcw, s.tcw), *s.cam)
        self.inf = ctx.size_sigma(kps)[2]

    def close(self):
        self.frame.close()
        self.points.close()


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return a.shape == b.shape and bool(np.all((a.view(np.uint8).reshape(a.shape + (-1,)) == b.view(np.uint8).reshape(b.shape + (-1,))).all(-1) |
                                                  (np.isnan(a) & np.isnan(b))))
    return np.array_equal(a, b)


def assert_equal(got, want, tag):
    assert got["n_edges"] == want.n_edges and got["rounds"] == want.rounds and got["n_good"] == want.n_good, (
        tag, got["n_edges"], want.n_edges, got["rounds"], want.rounds, got["n_good"], want.n_good)
    assert np.array_equal(got["iterations"], want.iterations) and np.array_equal(got["trials"], want.trials), (tag, got["iterations"], want.iterations,
                                                                                                               got["trials"], want.trials)
    assert same_bits(got["chi2"], want.chi2), (tag, got["chi2"], want.chi2)
    assert same_bits(got["lam"], want.lam), (tag, got["lam"], want.lam)
    assert same_bits(got["Rcw"].reshape(9), want.Rcw) and same_bits(got["tcw"], want.tcw), (tag, got["Rcw"], want.Rcw, got["tcw"], want.tcw)
    assert np.array_equal(got["outlier"], want.outlier != 0), tag


@pytest.mark.parametrize("case", CONSTRUCTED, ids=[s.name for s, _ in CONSTRUCTED])
def test_constructed_scene(afv, gpu_ctx, case):
    s, _ = case
    rig = Rig(afv, gpu_ctx, s)
    try:
        got = rig.frame.PoseOptimizationBatch(rig.points, [s.pts])[0]
        assert_equal(got, s.run(inf=rig.inf), s.name)
    finally:
        rig.close()


@pytest.mark.parametrize("n", SIZES)
def test_random_scene(afv, gpu_ctx, n):
    for kind in (("mixed",) if n > 2047 else ("mixed", "mono", "stereo")):
        s = S.random_scene(n % 7, n, kind)
        rig = Rig(afv, gpu_ctx, s)
        try:
            got = rig.frame.PoseOptimizationBatch(rig.points, [s.pts])[0]
            want = s.run(inf=rig.inf)
            assert_equal(got, want, (n, kind))
            if n >= 1023:
                assert want.rounds == 4 and want.n_good > n // 2
        finally:
            rig.close()


@pytest.mark.parametrize("njobs", (2, 7, 33))
def test_batches_equal_single_calls(afv, gpu_ctx, njobs):
    s = S.random_scene(3, 300)
    rig = Rig(afv, gpu_ctx, s)
    try:
        rs = np.random.RandomState(njobs)
        jobs = []
        for j in range(njobs):
            pts = np.where(rs.rand(s.N) < 0.8, s.pts, -1).astype(np.int32)
            Rj = (S.rot(rs.normal(0, 0.01, 3)) @ s.Rcw.astype(np.float64)).astype(np.float32)
            tj = (s.tcw + rs.normal(0, 0.02, 3)).astype(np.float32)
            jobs.append(pts if j == 0 else (pts, Rj, tj))
        got = rig.frame.PoseOptimizationBatch(rig.points, jobs)
        assert len(got) == njobs
        for j, job in enumerate(jobs):
            pts, Rj, tj = (job, s.Rcw, s.tcw) if j == 0 else job
            want = R.pose_optimization(s.problem(inf=rig.inf, pts=pts), Rj, tj)
            assert_equal(got[j], want, (njobs, j))
            single = rig.frame.PoseOptimizationBatch(rig.points, [job])[0]
            assert_equal(single, want, (njobs, j, "single"))
            for key in ("Rcw", "tcw", "chi2", "lam", "outlier", "iterations", "trials"):
                assert same_bits(single[key], got[j][key]), (njobs, j, key)
        assert len({g["Rcw"].tobytes() for g in got}) == njobs   # the jobs differ
    finally:
        rig.close()


def test_store_updated_between_two_calls(afv, gpu_ctx):
    s = S.random_scene(4, 200)
    rig = Rig(afv, gpu_ctx, s)
    try:
        first = rig.frame.PoseOptimizationBatch(rig.points, [s.pts])[0]
        assert_equal(first, s.run(inf=rig.inf), "before")
        pos, is_set = s.store_pos.copy(), s.store_set.copy()
        moved = s.pts[(s.pts >= 0) & s.store_set[np.clip(s.pts, 0, None)]][:40]
        pos[moved] += np.float32(0.01)
        never = s.pts[(s.pts >= 0) & ~s.store_set[np.clip(s.pts, 0, None)]]
        assert len(never) > 0
        is_set[never] = True                    # ids that were no points become edges
        rig.points.set(np.concatenate([moved, never]), pos=pos[np.concatenate([moved, never])])
        second = rig.frame.PoseOptimizationBatch(rig.points, [s.pts])[0]
        want = s.run(inf=rig.inf, store_pos=pos, store_set=is_set)
        assert_equal(second, want, "after")
        assert want.n_edges == first["n_edges"] + len(never) and not same_bits(second["Rcw"], first["Rcw"])
    finally:
        rig.close()


def test_chain_search_optimise_search(afv, gpu_ctx):
    """SearchLocalPoints -> PoseOptimization -> SearchLocalPoints with the pose staying in the library equals the same chain with the
    pose taken through the host (set_pose=False, then Frame.set_pose by the caller)"""
    import _points_ref as PR
    import _points_scenes as PS
    ps = PS.random_scene(1, PR.FRUSTUM)
    P, cam, f = ps.P, ps.cam, ps.feat
    results = []
    for through_host in (False, True):
        points = afv.MapPoints(gpu_ctx, P.capacity, desc_bytes=P.desc_bytes)
        ids = np.flatnonzero(P.flags & PR.SET)
        points.set(ids, pos=P.pos[ids], normal=P.normal[ids], min_distance=P.min_distance[ids], max_distance=P.max_distance[ids], ref_size=P.ref_size[ids],
                   ref_distance=P.ref_distance[ids], ref_sigma=P.ref_sigma[ids])
        points.set_flags(ids, bad=(P.flags[ids] & PR.BAD) != 0, observed=(P.flags[ids] & PR.OBSERVED) != 0)
        points.set_descriptors(ids, P.descriptors[ids])
        frame = afv.Frame(gpu_ctx, max_x=PS.W, max_y=PS.H, cap=f.n)
        kps = np.zeros(f.n, afv.KP_DTYPE)
        kps["x"], kps["y"], kps["angle"] = f.x, f.y, f.angles
        frame.set_features(kps, f.desc, sizes=f.sizes, u_right=f.u_right)
        frame.set_pose(cam.Rcw, cam.tcw, cam.Ow, cam.fx, cam.fy, cam.cx, cam.cy, cam.mbf)
        afv.FeatureMatcher.setDescriptorDistanceThresholds(ps.th)
        try:
            m = afv.FeatureMatcher(ps.nnratio, False, ctx=gpu_ctx)
            a1, n1, _ = frame.SearchLocalPoints(m, points, ps.ids, ps.radius_th, ps.cos_limit)
            pts = np.where(a1 >= 0, np.asarray(ps.ids)[np.clip(a1, 0, None)], -1).astype(np.int32)
            if through_host:
                ng, outl, Tcw = frame.PoseOptimization(points, pts, set_pose=False)
                Rn, tn = Tcw[:3, :3].copy(), Tcw[:3, 3].copy()
                frame.set_pose(Rn, tn, twc(Rn, tn), cam.fx, cam.fy, cam.cx, cam.cy, cam.mbf)
            else:
                ng, outl, Tcw = frame.PoseOptimization(points, pts)
            a2, n2, iv2 = frame.SearchLocalPoints(m, points, ps.ids, ps.radius_th, ps.cos_limit)
            results.append((a1, n1, ng, outl, Tcw, a2, n2, iv2))
        finally:
            afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)
            frame.close()
            points.close()
    a, b = results
    assert a[1] >= 5 and a[2] >= 3
    for u, v in zip(a, b):
        assert same_bits(u, v)
    assert not same_bits(a[4][:3, :3], np.asarray(cam.Rcw, np.float32).reshape(3, 3)) or not same_bits(a[4][:3, 3], np.asarray(cam.tcw, np.float32))


def test_refusals_before_any_launch(afv, gpu_ctx):
    L = afv._lib
    lib = L.load()
    s = S.random_scene(5, 50)
    rig = Rig(afv, gpu_ctx, s)
    other = afv.Context(max_width=640, max_height=480, max_batch=1)
    try:
        pts = np.ascontiguousarray(s.pts, np.int32)

        def call(frame=rig.frame, points=rig.points, p=pts, Rp=None, tp=None, njobs=1, job_size=None, res_size=None):
            J = (L.PoseJob * 65)()
            Rr = (L.PoseResult * 65)()
            for j in range(65):
                J[j].struct_size = C.sizeof(L.PoseJob) if job_size is None else job_size
                J[j].pts, J[j].Rcw, J[j].tcw = L.ptr(p), L.ptr(Rp), L.ptr(tp)
                Rr[j].struct_size = C.sizeof(L.PoseResult) if res_size is None else res_size
            return lib.afv_frame_pose_optimize(frame.handle, points.handle, J, njobs, Rr)

        assert call() == L.OK
        assert call(njobs=0) == L.EINVAL and call(njobs=65) == L.EINVAL and call(njobs=64) == L.OK
        assert call(job_size=8) == L.EINVAL and call(job_size=0) == L.EINVAL and call(res_size=16) == L.EINVAL
        assert call(p=None) == L.EINVAL
        assert call(Rp=np.eye(3, dtype=np.float32).reshape(9)) == L.EINVAL          # a rotation without a translation
        beyond = pts.copy()
        beyond[3] = len(s.store_set)
        assert call(p=beyond) == L.EINVAL
        foreign = afv.MapPoints(other, 64)
        assert call(points=foreign) == L.EINVAL
        foreign.close()
        no_pose = afv.Frame(gpu_ctx, max_x=S.W, max_y=S.H, cap=s.N)
        kps = np.zeros(s.N, afv.KP_DTYPE)
        no_pose.set_features(kps, np.zeros((s.N, 32), np.uint8))
        assert call(frame=no_pose) == L.EINVAL
        no_pose.close()
        empty = afv.Frame(gpu_ctx, max_x=S.W, max_y=S.H, cap=4)
        empty.set_pose(s.Rcw, s.tcw, twc(s.Rcw, s.tcw), *s.cam)
        assert call(frame=empty) == L.EINVAL                                        # no features
        empty.close()
        wide = afv.MapPoints(gpu_ctx, len(s.store_set), desc_bytes=61)              # the descriptor kind of the store does not matter
        ids = np.flatnonzero(s.store_set)
        wide.set(ids, pos=s.store_pos[ids])
        got = rig.frame.PoseOptimizationBatch(wide, [s.pts])[0]
        assert_equal(got, s.run(inf=rig.inf), "another descriptor width")
        wide.close()
    finally:
        rig.close()
        other.close()


def test_cpp_adapter_pose_optimization(afv, gpu_ctx, tmp_path):
    assert os.path.exists(BIN), "poseopt_selftest is not built: __graft_entry__.build() compiles it"
    s = S.random_scene(2, 400)

    def hx(v):
        return float(np.float32(v)).hex()

    ids = np.flatnonzero(s.store_set)
    lines = ["%d %d" % (len(s.store_set), len(ids))]
    for i in ids:
        lines.append(" ".join([str(i)] + [hx(v) for v in s.store_pos[i]]))
    lines.append(" ".join(hx(v) for v in list(s.Rcw.reshape(9)) + list(s.tcw) + list(twc(s.Rcw, s.tcw)) + list(s.cam)))
    lines.append("%s %s %d" % (hx(S.W), hx(S.H), s.N))
    for k in range(s.N):
        lines.append(" ".join([hx(s.x[k]), hx(s.y[k]), hx(s.u_right[k]), str(int(s.octave[k])), str(int(s.pts[k]))]))
    inp = tmp_path / "scene.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([BIN, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = {l.split(":")[0]: l.split(":")[1].split() for l in r.stdout.splitlines()}
    rig = Rig(afv, gpu_ctx, s)
    try:
        want = s.run(inf=rig.inf)
    finally:
        rig.close()
    assert int(got["ngood"][0]) == want.n_good and want.n_good >= 100
    pose = np.array([float.fromhex(v) for v in got["pose"]], np.float32)
    assert same_bits(pose[:9], want.Rcw) and same_bits(pose[9:], want.tcw)
    assert np.array_equal(np.array(got["outlier"], np.int64), want.outlier)
    # the pose went back into the frame: the next projection of the adapter runs on it
    stored = np.array([float.fromhex(v) for v in got["stored"]], np.float32)
    assert same_bits(stored[:9], want.Rcw) and same_bits(stored[9:12], want.tcw) and same_bits(stored[12:], twc(want.Rcw.reshape(3, 3), want.tcw))
