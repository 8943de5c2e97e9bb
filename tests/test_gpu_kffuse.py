"""-m gpu: afv_table_fuse_points (Fuse into keyframes of the table) against the restatement tests/_kffuse_ref.py, bit for bit on best, occupant,
status and nfused: the constructed scenes and the seeded random maps of tests/_kffuse_scenes.py (query counts, features per slot and
target counts at and around the kernels' block and wavefront sizes; binary rows of 32 and 61 bytes, float rows of 128; mono and stereo
slots; both flavours; shared and per-target lists; an empty job in the middle; pose_override), agreement with Frame.FusePoints on a resident
frame, a promoted slot, the lifetime of the slot's grid, clone_into, every refusal with outputs and store unchanged, and the Python mirrors
on a small map.  tests/test_kffuse_ref_cpu.py proves on the CPU that every scene reaches the rule it is named after."""
import copy
import ctypes as C

import numpy as np
import pytest

import _kffuse_ref as K
import _kffuse_scenes as KS
import _points_ref as R

pytestmark = pytest.mark.gpu

CASES = KS.all_constructed()
_maps = {}


def the_map(*key, **kw):
    k = (key, tuple(sorted(kw.items())))
    if k not in _maps:
        _maps[k] = KS.random_map(*key, **kw)
    return _maps[k]


def fill_store(points, P):
    ids = np.flatnonzero(P.flags & R.SET).astype(np.int32)
    points.set(ids, pos=P.pos[ids], normal=P.normal[ids], min_distance=P.min_distance[ids], max_distance=P.max_distance[ids],
               ref_size=P.ref_size[ids], ref_distance=P.ref_distance[ids], ref_sigma=P.ref_sigma[ids])
    points.set_flags(ids, bad=P.flags[ids] & R.BAD, observed=P.flags[ids] & R.OBSERVED)
    points.set_descriptors(ids, P.descriptors[ids])
    odd = np.flatnonzero((P.flags & R.SET == 0) & (P.flags & R.BAD != 0)).astype(np.int32)   # never set, yet flagged bad
    if len(odd):
        points.set_flags(odd, bad=np.ones(len(odd), np.uint8))


def fill_slot(table, s, kf, pose=True, plane=True):
    table.set(s, kf.desc)
    table.set_geometry(s, kf.x, kf.y, kf.sizes * kf.sizes, u_right=kf.u_right)
    table.set_scale(s, kf.sizes)
    table.set_inf(s, kf.inf)
    c = kf.cam
    if pose:
        table.set_pose(s, c.Rcw, c.tcw, c.Ow, c.fx, c.fy, c.cx, c.cy, c.mbf)
    if plane:
        table.set_map_points(s, kf.plane)


def set_camera(table, g):
    table.set_camera(g.min_x, g.max_x, g.min_y, g.max_y, g.cols, g.rows, g.inv_w, g.inv_h)


class Rig:
    def __init__(self, afv, ctx, P, kfs, grid, nsets=None, cap=None):
        self.afv, self.P, self.kfs = afv, P, kfs
        self.points = afv.MapPoints(ctx, P.capacity, desc_bytes=P.desc_bytes, float_dim=P.float_dim)
        fill_store(self.points, P)
        nsets = max(kfs) + 1 if nsets is None else nsets
        cap = max(max(kf.n for kf in kfs.values()), 1) if cap is None else cap
        kind = dict(float_dim=P.float_dim) if P.float_dim else dict(desc_bytes=P.desc_bytes)
        self.table = afv.table.DescriptorTable(ctx, nsets, cap, **kind)
        set_camera(self.table, grid)
        for s, kf in kfs.items():
            fill_slot(self.table, s, kf)

    def close(self):
        self.table.close()
        self.points.close()


def call(rig, jobs):
    """jobs as tests/_kffuse_ref.fuse_batch takes them -> the device's answer in the same shape"""
    t = rig.table
    by_flavour = {}
    for k, j in enumerate(jobs):
        by_flavour.setdefault((j.get("use_inf_gate", True), j.get("pose") is not None, float(j.get("radius_th", 3.0)), float(j.get("th_low", KS.TH))), []).append(k)
    assert len(by_flavour) == 1, "one flavour per call of the wrapper"
    (gate, over, rth, th), _ = next(iter(by_flavour.items()))
    return t._fuse(rig.points, [j["slot"] for j in jobs], [j["ids"] for j in jobs], rth, th, gate, [j["pose"] for j in jobs] if over else None)


def assert_same(got, want, name=""):
    for k in range(len(want[0])):
        for a, b, what in zip(got[:3], want[:3], ("best", "occupant", "status")):
            assert np.array_equal(a[k], b[k]), (name, "job %d" % k, what, a[k], b[k])
    assert np.array_equal(got[3], want[3]), (name, "nfused", got[3], want[3])


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_constructed_scene(afv, gpu_ctx, c):
    rig = Rig(afv, gpu_ctx, c.P, c.kfs, c.grid)
    try:
        res = c.run()
        want = ([r[0] for r in res], [r[1] for r in res], [r[2] for r in res], np.array([r[3] for r in res], np.int32))
        jobs = [dict(j, th_low=j.get("th_low", KS.TH)) for j in c.jobs]
        assert_same(call(rig, jobs), want, c.name)
    finally:
        rig.close()


def run_map(afv, ctx, m, gate=True, poses=None, cap=None):
    rig = Rig(afv, ctx, m.P, m.kfs, m.grid, cap=cap)
    try:
        jobs = [dict(slot=s, ids=m.lists[s], th_low=m.th_low, use_inf_gate=gate, pose=None if poses is None else poses[s]) for s in sorted(m.kfs)]
        got = call(rig, jobs)
        want = KS.expected(m, gate, poses)
        assert_same(got, want, m.name)
        return want
    finally:
        rig.close()


# (nq, features per slot, targets): the block of 256 queries, the wavefront of 64, a slot of one feature, many blocks, many targets
SHAPES = [(0, 64, 1), (1, 64, 1), (63, 65, 7), (64, 64, 1), (65, 1, 1), (1000, 1000, 2), (65, 65, 64)]


@pytest.mark.parametrize("nq,nf,nt", SHAPES, ids=["q%d_f%d_t%d" % s for s in SHAPES])
def test_random_map_shapes(afv, gpu_ctx, nq, nf, nt):
    want = run_map(afv, gpu_ctx, the_map(1, nq, nf, nt))
    if nq >= 63:
        seen = set(int(v) for st in want[2] for v in st)
        assert {K.INVALID, K.NOT_IN_VIEW, K.FREE} <= seen, seen


def test_slot_filled_to_its_cap(afv, gpu_ctx):
    run_map(afv, gpu_ctx, the_map(2, 200, 256, 1), cap=256)


KINDS = [("binary61", dict(desc_bytes=61)), ("float128", dict(float_dim=128)), ("stereo32", dict(stereo=True)), ("per_target_lists", dict(per_target=True))]


@pytest.mark.parametrize("gate", (True, False), ids=("inf_gate", "no_gate"))
@pytest.mark.parametrize("name,kw", KINDS, ids=[k[0] for k in KINDS])
def test_random_map_kinds(afv, gpu_ctx, name, kw, gate):
    want = run_map(afv, gpu_ctx, the_map(3, 130, 90, 3, **kw), gate=gate)
    assert sum(int(n) for n in want[3]) > 0


def test_pose_override_sim3(afv, gpu_ctx):
    m = the_map(4, 130, 90, 3, stereo=True)
    poses = {}
    for s, kf in m.kfs.items():
        Scw = np.eye(4, dtype=np.float32)
        Scw[:3, :3] = kf.cam.Rcw * np.float32(1.0 + 0.1 * s)
        Scw[:3, 3] = kf.cam.tcw
        poses[s] = K.decompose_scw(Scw)
    want = run_map(afv, gpu_ctx, m, gate=False, poses=poses)
    assert sum(int(n) for n in want[3]) > 0
    # ... and through the wrapper that decomposes Scw itself
    rig = Rig(afv, gpu_ctx, m.P, m.kfs, m.grid)
    try:
        Scw = []
        for s in sorted(m.kfs):
            S = np.eye(4, dtype=np.float32)
            S[:3, :3] = m.kfs[s].cam.Rcw * np.float32(1.0 + 0.1 * s)
            S[:3, 3] = m.kfs[s].cam.tcw
            Scw.append(S)
        got = rig.table.FusePointsSim3(rig.points, sorted(m.kfs), Scw, m.lists[0], radiusTh=3.0, th_low=m.th_low)
        assert_same(got, want, "FusePointsSim3")
    finally:
        rig.close()


def test_shared_and_own_lists_and_an_empty_job_in_one_call(afv, gpu_ctx):
    m = the_map(5, 100, 80, 4)
    rig = Rig(afv, gpu_ctx, m.P, m.kfs, m.grid)
    try:
        shared = np.ascontiguousarray(m.lists[0], np.int32)
        own = np.ascontiguousarray(shared[::-1][:37])
        empty = np.zeros(0, np.int32)
        lists = [shared, own, empty, shared, shared[:64].copy()]
        slots = [0, 1, 2, 3, 1]
        got = rig.table.FusePoints(rig.points, slots, lists, radiusTh=3.0, th_low=m.th_low)
        want = K.fuse_batch(m.P, m.kfs, m.grid, [dict(slot=s, ids=a, th_low=m.th_low) for s, a in zip(slots, lists)])
        assert_same(got, want, "mixed lists")
        assert len(got[0][2]) == 0 and got[3][2] == 0
        # one list for all targets: the call of SearchInNeighbors' first half
        got = rig.table.FusePoints(rig.points, [0, 1, 2, 3], shared, radiusTh=3.0, th_low=m.th_low)
        assert_same(got, KS.expected(m), "one list")
        # the answer does not change when it is asked again (the grids are kept) and nothing was written
        assert_same(rig.table.FusePoints(rig.points, [0, 1, 2, 3], shared, radiusTh=3.0, th_low=m.th_low), KS.expected(m), "again")
        for s, kf in m.kfs.items():
            assert np.array_equal(rig.table.get_map_points(s, kf.n), kf.plane)
    finally:
        rig.close()


def test_best_equals_frame_fuse_points(afv, gpu_ctx):
    """the two entry points agree: a resident frame given the features, pose and ids of a slot whose plane is empty"""
    m = copy.deepcopy(the_map(6, 130, 90, 1, stereo=True))
    kf = m.kfs[0]
    kf.plane[:] = -1
    rig = Rig(afv, gpu_ctx, m.P, m.kfs, m.grid)
    fr = afv.Frame(gpu_ctx, max_x=96.0, max_y=64.0, cap=kf.n, desc_bytes=m.P.desc_bytes)
    try:
        kps = np.zeros(kf.n, afv.KP_DTYPE)
        kps["x"], kps["y"] = kf.x, kf.y
        fr.set_features(kps, kf.desc, sizes=kf.sizes, u_right=kf.u_right)
        c = kf.cam
        fr.set_pose(c.Rcw, c.tcw, c.Ow, c.fx, c.fy, c.cx, c.cy, c.mbf)
        afv.FeatureMatcher.setDescriptorDistanceThresholds(m.th_low)
        for gate in (True, False):
            want, n = fr.FusePoints(afv.FeatureMatcher(0.8, False, ctx=gpu_ctx), rig.points, m.lists[0], 3.0, use_inf_gate=gate)
            best, _, st, nf = rig.table._fuse(rig.points, [0], m.lists[0], 3.0, m.th_low, gate, None)
            assert np.array_equal(best[0], want) and nf[0] == n and n > 0
    finally:
        afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)
        fr.close()
        rig.close()


def test_promoted_slot(afv, gpu_ctx):
    """KeyFrame::KeyFrame(Frame&): a slot filled by set_from_frame answers like the same slot filled from host arrays; the promotion forgets
    the pose and the plane of the slot's previous occupant"""
    m = the_map(7, 100, 70, 2)
    rig = Rig(afv, gpu_ctx, m.P, m.kfs, m.grid)
    kf = m.kfs[1]
    fr = afv.Frame(gpu_ctx, max_x=96.0, max_y=64.0, cap=kf.n)
    try:
        kps = np.zeros(kf.n, afv.KP_DTYPE)
        kps["x"], kps["y"] = kf.x, kf.y
        fr.set_features(kps, kf.desc, sizes=kf.sizes)
        rig.table.set_from_frame(1, fr)
        L = afv._lib
        with pytest.raises(L.AfvError) as e:
            rig.table.FusePoints(rig.points, [1], m.lists[1], th_low=m.th_low)
        assert e.value.code == L.EINVAL
        c = kf.cam
        rig.table.set_pose(1, c.Rcw, c.tcw, c.Ow, c.fx, c.fy, c.cx, c.cy, c.mbf)
        rig.table.set_map_points(1, kf.plane)
        assert_same(rig.table.FusePoints(rig.points, [0, 1], m.lists[0], th_low=m.th_low), KS.expected(m), "promoted")
    finally:
        fr.close()
        rig.close()


def test_grid_follows_geometry_scale_and_camera(afv, gpu_ctx):
    m = copy.deepcopy(the_map(8, 100, 70, 1))
    rig = Rig(afv, gpu_ctx, m.P, m.kfs, m.grid)
    kf = m.kfs[0]
    try:
        ask = lambda: rig.table.FusePoints(rig.points, [0], m.lists[0], th_low=m.th_low)
        first = KS.expected(m)
        assert_same(ask(), first, "before")
        # the features move: mirrored in x
        kf.x = (np.float32(96.0) - kf.x).astype(np.float32)
        rig.table.set_geometry(0, kf.x, kf.y, kf.sizes * kf.sizes)
        moved = KS.expected(m)
        assert not np.array_equal(moved[0][0], first[0][0])
        assert_same(ask(), moved, "after set_geometry")
        # their sizes change: the entries of the grid carry keyPtsSize
        kf.x = (np.float32(96.0) - kf.x).astype(np.float32)
        rig.table.set_geometry(0, kf.x, kf.y, kf.sizes * kf.sizes)
        kf.sizes = (kf.sizes * np.float32(1.3)).astype(np.float32)
        rig.table.set_scale(0, kf.sizes)
        sized = KS.expected(m)
        assert not np.array_equal(sized[0][0], first[0][0])
        assert_same(ask(), sized, "after set_scale")
        # another grid and narrower bounds
        m.grid = K.Grid(8.0, 90.0, 4.0, 60.0, 16, 9)
        set_camera(rig.table, m.grid)
        cam = KS.expected(m)
        assert not np.array_equal(cam[2][0], sized[2][0])
        assert_same(ask(), cam, "after set_camera")
    finally:
        rig.close()


def test_pose_and_plane_survive_clone_into(afv, gpu_ctx):
    m = the_map(9, 100, 70, 3)
    rig = Rig(afv, gpu_ctx, m.P, m.kfs, m.grid)
    other = afv.table.DescriptorTable(gpu_ctx, rig.table.nsets, rig.table.cap)
    try:
        rig.table.clone_into(other)
        for s, kf in m.kfs.items():
            assert np.array_equal(other.get_map_points(s, kf.n), kf.plane)
        assert_same(other.FusePoints(rig.points, sorted(m.kfs), m.lists[0], th_low=m.th_low), KS.expected(m), "clone")
        # afv_table_set forgets both
        other.set(1, m.kfs[1].desc)
        L = afv._lib
        with pytest.raises(L.AfvError) as e:
            other.get_map_points(1, m.kfs[1].n)
        assert e.value.code == L.EINVAL
    finally:
        other.close()
        rig.close()


def test_refusals_leave_outputs_and_store_unchanged(afv, gpu_ctx):
    L = afv._lib
    lib = L.load()
    m = the_map(10, 60, 50, 3)
    rig = Rig(afv, gpu_ctx, m.P, m.kfs, m.grid, nsets=8)
    ids = np.ascontiguousarray(m.lists[0], np.int32)
    nq = len(ids)
    store_ids = np.flatnonzero(m.P.flags & R.SET).astype(np.int32)
    before = rig.points.get(store_ids)
    extra = []

    def attempt(t=None, p=None, nt=1, ss=None, **over):
        jobs = (L.TableFuseJob * 65)()
        for k in range(65):
            j = jobs[k]
            j.struct_size = C.sizeof(L.TableFuseJob) if ss is None else ss
            j.slot, j.ids, j.nq = 0, ids.ctypes.data, nq
            j.radius_th, j.radius_scale, j.th_low, j.use_inf_gate = 3.0, 1.15, m.th_low, 1
        for k, v in over.items():
            setattr(jobs[0], k, v)
        best, occ = np.full(65 * nq, 77, np.int32), np.full(65 * nq, 77, np.int32)
        st, nf = np.full(65 * nq, 0xA5, np.uint8), np.full(65, 77, np.int32)
        code = lib.afv_table_fuse_points((rig.table if t is None else t).handle, (rig.points if p is None else p).handle, jobs, nt, L.ptr(best),
                                         L.ptr(occ), L.ptr(st), L.ptr(nf))
        return code, bool(np.all(best == 77) and np.all(occ == 77) and np.all(st == 0xA5) and np.all(nf == 77))

    def bare(**skip):
        """a table with slot 0 filled but for one thing"""
        t = afv.table.DescriptorTable(gpu_ctx, 2, rig.table.cap)
        extra.append(t)
        kf = m.kfs[0]
        if not skip.get("camera"):
            set_camera(t, m.grid)
        t.set(0, kf.desc)
        if not skip.get("geometry"):
            t.set_geometry(0, kf.x, kf.y, kf.sizes * kf.sizes)
            if not skip.get("scale"):
                t.set_scale(0, kf.sizes)
            if not skip.get("inf"):
                t.set_inf(0, kf.inf)
        fill = kf.cam
        if not skip.get("pose"):
            t.set_pose(0, fill.Rcw, fill.tcw, fill.Ow, fill.fx, fill.fy, fill.cx, fill.cy, fill.mbf)
        if not skip.get("plane"):
            t.set_map_points(0, kf.plane)
        return t

    try:
        assert attempt() == (0, False)                                  # the call itself is good
        assert attempt(nt=0) == (0, True)                               # nt == 0 is legal and touches nothing
        assert attempt(nt=-1) == (L.EINVAL, True)
        assert attempt(nt=65) == (L.EINVAL, True)
        assert attempt(nt=64)[0] == 0
        assert attempt(slot=-1) == (L.EINVAL, True)
        assert attempt(slot=8) == (L.EINVAL, True)
        assert attempt(slot=5) == (L.EINVAL, True)                      # a slot that was never filled
        for what in ("geometry", "scale", "inf", "plane", "pose", "camera"):
            assert attempt(t=bare(**{what: True})) == (L.EINVAL, True), what
        assert attempt(t=bare())[0] == 0
        assert attempt(t=bare(inf=True), use_inf_gate=0)[0] == 0        # Fuse no. 2 reads no information plane
        over = L.TableFusePose()
        assert attempt(t=bare(pose=True), pose_override=C.pointer(over))[0] == L.EINVAL  # (the intrinsics are the slot's pose's)
        ctx2 = afv.Context(max_width=640, max_height=480, max_batch=1)
        p2 = afv.MapPoints(ctx2, m.P.capacity)
        extra.append(p2)
        assert attempt(p=p2) == (L.EINVAL, True)                        # store and table on different contexts
        for kind in (dict(desc_bytes=61), dict(float_dim=32), dict(float_dim=8)):
            p3 = afv.MapPoints(gpu_ctx, m.P.capacity, **kind)
            extra.append(p3)
            assert attempt(p=p3) == (L.EUNSUPPORTED, True), kind
        bad_ids = ids.copy()
        bad_ids[nq // 2] = m.P.capacity
        assert attempt(ids=bad_ids.ctypes.data) == (L.EINVAL, True)
        bad_ids[nq // 2] = -2
        assert attempt(ids=bad_ids.ctypes.data) == (L.EINVAL, True)
        assert attempt(nq=65536) == (L.EINVAL, True)
        assert attempt(nq=-1) == (L.EINVAL, True)
        assert attempt(ids=None) == (L.EINVAL, True)
        assert attempt(use_inf_gate=2) == (L.EINVAL, True)
        for ss in (0, 8, C.sizeof(L.TableFuseJob) - 4, C.sizeof(L.TableFuseJob) + 2, 5 * C.sizeof(L.TableFuseJob)):
            assert attempt(ss=ss) == (L.EINVAL, True), ss
        # a query total beyond the cap: 17 jobs of 65535 ids
        big = np.full(65535, -1, np.int32)
        jobs = (L.TableFuseJob * 17)()
        for j in jobs:
            j.struct_size = C.sizeof(L.TableFuseJob)
            j.slot, j.ids, j.nq, j.radius_th, j.radius_scale, j.th_low, j.use_inf_gate = 0, big.ctypes.data, 65535, 3.0, 1.15, m.th_low, 1
        outs = np.full(4, 77, np.int32), np.full(4, 77, np.int32), np.full(4, 0xA5, np.uint8), np.full(17, 77, np.int32)
        assert lib.afv_table_fuse_points(rig.table.handle, rig.points.handle, jobs, 17, *[L.ptr(a) for a in outs]) == L.EINVAL
        assert all(np.all(a == (0xA5 if a.dtype == np.uint8 else 77)) for a in outs)
        # the setters' own refusals
        cam = L.sized(L.TableCamera)
        cam.max_x, cam.max_y, cam.grid_cols, cam.grid_rows, cam.grid_inv_w, cam.grid_inv_h = 96.0, 64.0, 128, 65, 1.0, 1.0
        assert lib.afv_table_set_camera(rig.table.handle, C.byref(cam)) == L.EINVAL        # 8320 cells
        cam.grid_rows, cam.struct_size = 48, 12
        assert lib.afv_table_set_camera(rig.table.handle, C.byref(cam)) == L.EINVAL
        assert lib.afv_table_set_map_points(rig.table.handle, 8, L.ptr(ids)) == L.EINVAL
        assert lib.afv_table_get_map_points(rig.table.handle, 5, L.ptr(ids)) == L.EINVAL
        # nothing of it reached the store or the planes
        after = rig.points.get(store_ids)
        for k in before:
            assert before[k].tobytes() == after[k].tobytes(), k
        for s, kf in m.kfs.items():
            assert np.array_equal(rig.table.get_map_points(s, kf.n), kf.plane)
        assert_same(rig.table.FusePoints(rig.points, sorted(m.kfs), ids, th_low=m.th_low), KS.expected(m), "after the refusals")
    finally:
        for o in extra:
            o.close()
        rig.close()


def test_python_mirrors_on_a_small_map(afv, gpu_ctx):
    """SearchInNeighborsFuse and SearchAndFuse with the toy map's surgery as the callback against the sequential restatement"""
    grid = K.Grid()
    for seed in range(2):
        P1, k1 = KS.small_map(seed)
        P2, k2 = copy.deepcopy((P1, k1))
        Ma = K.ToyMap(P1, k1)
        want = K.search_in_neighbors(Ma, grid, 0, [1, 2], th_low=KS.TH)
        rig = Rig(afv, gpu_ctx, P2, k2, grid)
        try:
            Mb = K.ToyMap(P2, k2)

            def on_fuse(s, ids, best, occ, status, sim3=False):
                Mb.apply(s, ids, best, status, sim3=sim3)
                every = np.arange(17, dtype=np.int32)
                rig.points.set_flags(every, bad=P2.flags[every] & R.BAD)      # what the surgery changed: flags and planes
                for t, kf in k2.items():
                    rig.table.set_map_points(t, kf.plane)
            got = rig.table.SearchInNeighborsFuse(rig.points, 0, [1, 2], lambda: k2[0].plane.copy(), lambda s: k2[s].plane.copy(), on_fuse,
                                                  th_low=KS.TH)
            assert (got[0], got[1]) == want and sum(want[0]) > 0
            assert Ma.lists() == Mb.lists()
            for s in k1:
                assert np.array_equal(rig.table.get_map_points(s, k1[s].n), k1[s].plane)
            # SearchAndFuse on the fused map: corrected poses = the keyframes' own
            Scw = []
            for s in (1, 2):
                S = np.eye(4, dtype=np.float32)
                S[:3, 3] = k1[s].cam.tcw
                Scw.append(S)
            loop_ids = list(range(17))
            want2 = K.search_and_fuse(Ma, grid, [1, 2], Scw, loop_ids, th_low=KS.TH)
            got2 = rig.table.SearchAndFuse(rig.points, [1, 2], Scw, loop_ids, lambda *a: on_fuse(*a, sim3=True), th_low=KS.TH)
            assert got2 == want2 and Ma.lists() == Mb.lists()
        finally:
            rig.close()


def test_cpp_adapter_answers_as_the_restatement(afv, gpu_ctx, tmp_path):
    """afv::FuseIntoKeyFrames / afv::FuseIntoKeyFramesSim3 (adapter/kffuse_selftest) as a plain C++ process on one small stereo map: one
    shared list into three keyframes, both flavours; the adapter decomposes Scw in its own text"""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "anyfeature-vslam_amd", "adapter", "kffuse_selftest")
    assert os.path.exists(exe), "kffuse_selftest is not built: __graft_entry__.build() compiles it"
    m = the_map(11, 90, 70, 3, stereo=True)
    hx = lambda v: float(np.float32(v)).hex()
    P, g = m.P, m.grid
    ids = np.flatnonzero(P.flags & R.SET)
    slots = sorted(m.kfs)
    Scw = {}
    for s in slots:
        S = np.eye(4, dtype=np.float32)
        S[:3, :3] = m.kfs[s].cam.Rcw * np.float32(1.0 + 0.2 * s)
        S[:3, 3] = m.kfs[s].cam.tcw + np.float32(0.01 * s)
        Scw[s] = S
    lines = ["%d %d %d %d %d %s" % (max(kf.n for kf in m.kfs.values()), len(slots), P.capacity, len(ids), len(m.lists[0]), hx(m.th_low)),
             "%s %s %s %s %d %d %s %s" % (hx(g.min_x), hx(g.max_x), hx(g.min_y), hx(g.max_y), g.cols, g.rows, hx(g.inv_w), hx(g.inv_h))]
    for s in slots:
        kf, c = m.kfs[s], m.kfs[s].cam
        lines.append("%d %d" % (s, kf.n))
        lines.append(" ".join(hx(v) for v in list(c.Rcw.reshape(9)) + list(c.tcw) + [c.fx, c.fy, c.cx, c.cy, c.mbf]))
        lines.append(" ".join(hx(v) for v in Scw[s].reshape(16)))
        lines += ["%s %s %s %s %s %d %s" % (hx(kf.x[i]), hx(kf.y[i]), hx(kf.u_right[i]), hx(kf.inf[i]), hx(kf.sizes[i]), kf.plane[i],
                                            kf.desc[i].tobytes().hex()) for i in range(kf.n)]
    for i in ids:
        vals = list(P.pos[i]) + list(P.normal[i]) + [P.min_distance[i], P.max_distance[i], P.ref_size[i], P.ref_distance[i], P.ref_sigma[i]]
        lines.append("%d %s %d %s" % (i, " ".join(hx(v) for v in vals), 1 if P.flags[i] & R.BAD else 0, P.descriptors[i].tobytes().hex()))
    lines.append(" ".join(str(int(v)) for v in m.lists[0]))
    inp = tmp_path / "map.txt"
    inp.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = []
    for tag, gate, poses in (("F", True, None), ("S", False, {s: K.decompose_scw(Scw[s]) for s in slots})):
        jobs = [dict(slot=s, ids=m.lists[0], th_low=m.th_low, use_inf_gate=gate, pose=None if poses is None else poses[s],
                     radius_th=3.0 if gate else 4.0) for s in slots]
        best, occ, st, nf = K.fuse_batch(P, m.kfs, g, jobs)
        assert nf.sum() > 0
        for k, s in enumerate(slots):
            want.append("%s %d %d" % (tag, s, nf[k]))
            want += ["%d %d %d" % (best[k][q], occ[k][q], st[k][q]) for q in range(len(m.lists[0]))]
    assert [l.rstrip() for l in r.stdout.splitlines()] == want
