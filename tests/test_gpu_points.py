"""-m gpu: the resident map points (afv_points_*, afv_frame_set_pose, afv_frame_project_points / _search_points / _fuse_points) against the
restatement tests/_points_ref.py on the constructed and the seeded random scenes of tests/_points_scenes.py - floats as bits, in_view and the
count exactly - and the searches against two things that must agree: the restatement composed with tests/_proj_ref.py, and the host-array
entry points afv_frame_match_projection / _fuse fed with the restatement's queries.  tests/test_points_ref_cpu.py proves on the CPU that
every scene reaches the rule it is named after."""
import ctypes as C

import numpy as np
import pytest

import _points_ref as R
import _points_scenes as S
import _proj_ref as PR

pytestmark = pytest.mark.gpu

CASES = S.all_constructed()
SEARCH = [c for c in CASES if c.feat is not None]
RANDOM = [(seed, fl) for seed in range(3) for fl in (R.FRUSTUM, R.LASTFRAME, R.RELOC, R.FUSE)]
FLOATS = ("u", "v", "ur", "size", "sigma", "view_cos", "r", "qmin", "qmax", "er")
_scene_cache = {}


def random_scene(seed, fl):
    if (seed, fl) not in _scene_cache:
        _scene_cache[(seed, fl)] = S.random_scene(seed, fl)
    return _scene_cache[(seed, fl)]


class Rig:
    """a scene on the device: the store, the frame with its pose, the last frame where the flavour has one"""

    def __init__(self, afv, ctx, s, P=None, feat=None):
        P = s.P if P is None else P
        feat = s.feat if feat is None else feat
        self.afv, self.s = afv, s
        self.points = afv.MapPoints(ctx, P.capacity, desc_bytes=P.desc_bytes, float_dim=P.float_dim)
        fill_store(self.points, P)
        fl = bool(P.float_dim)
        self.frame = afv.Frame(ctx, max_x=S.W, max_y=S.H, cap=max(feat.n if feat else 1, 1), desc_bytes=P.desc_bytes, float_dim=P.float_dim)
        kps = np.zeros(feat.n if feat else 0, afv.KP_DTYPE)
        if feat:
            kps["x"], kps["y"], kps["angle"] = feat.x, feat.y, feat.angles
            self.frame.set_features(kps, feat.desc, sizes=feat.sizes, u_right=feat.u_right)
        else:
            self.frame.set_features(kps, np.zeros((0, P.float_dim if fl else P.desc_bytes), np.float32 if fl else np.uint8))
        cam = s.cam
        self.frame.set_pose(cam.Rcw, cam.tcw, cam.Ow, cam.fx, cam.fy, cam.cx, cam.cy, cam.mbf)
        self.last = None
        if s.flavour == R.LASTFRAME or (s.flavour == R.RELOC and s.last_angles is not None):
            n = len(s.ids)
            self.last = afv.Frame(ctx, max_x=S.W, max_y=S.H, cap=max(n, 1), desc_bytes=P.desc_bytes, float_dim=P.float_dim)
            lk = np.zeros(n, afv.KP_DTYPE)
            if s.last_angles is not None:
                lk["angle"] = s.last_angles
            rows = np.zeros((n, P.float_dim if fl else P.desc_bytes), np.float32 if fl else np.uint8)
            self.last.set_features(lk, rows, sizes=np.ones(n, np.float32) if s.last_sizes is None else s.last_sizes)

    def project(self, ids=None):
        s = self.s
        return self.frame.project_points(self.points, s.ids if ids is None else ids, s.flavour, radiusTh=s.radius_th,
                                         viewingCosLimit=s.cos_limit, last=self.last if s.flavour == R.LASTFRAME else None,
                                         radius_scale=s.radius_scale)

    def matcher(self):
        afv, s = self.afv, self.s
        afv.FeatureMatcher.setDescriptorDistanceThresholds(s.th)
        return afv.FeatureMatcher(s.nnratio, s.check_orientation, ctx=self.frame.ctx)

    def search(self, ids=None, host_angles=False):
        """-> (assign | best, count, in_view | None)"""
        s, m = self.s, self.matcher()
        ids = s.ids if ids is None else ids
        f = self.frame
        try:
            f.RADIUS_SCALE = float(s.radius_scale)
            if s.flavour == R.FRUSTUM:
                return f.SearchLocalPoints(m, self.points, ids, s.radius_th, s.cos_limit, occupied=s.occupied)
            if s.flavour == R.LASTFRAME:
                return f.SearchByProjectionLast(m, self.points, self.last, ids, s.radius_th, occupied=s.occupied) + (None,)
            if s.flavour == R.RELOC:
                if host_angles:   # the keyframe's angles as a host array instead of a resident frame in its role
                    return f.SearchByProjectionReloc(m, self.points, ids, s.radius_th, angles=s.last_angles[:len(ids)], occupied=s.occupied) + (None,)
                return f.SearchByProjectionReloc(m, self.points, ids, s.radius_th, keyframe=self.last, occupied=s.occupied) + (None,)
            return f.FusePoints(m, self.points, ids, s.radius_th, use_inf_gate=s.inf_gate) + (None,)
        finally:
            self.afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)

    def host_array_search(self, Q):
        """the same search through the host-array entry points, fed with the restatement's queries"""
        s, m = self.s, self.matcher()
        q = self.afv.ProjectionQueries(Q.descriptors, Q.u, Q.v, Q.r, Q.min_size, Q.max_size, valid=Q.valid, angles=Q.angles, occupies=Q.occupies,
                                       ur=Q.ur, er_max=Q.er_max)
        try:
            if s.flavour == R.FUSE:
                return self.frame.Fuse(m, q, use_inf_gate=s.inf_gate)
            if s.flavour == R.FRUSTUM:
                m.mbCheckOrientation = False
            if s.flavour == R.RELOC:   # (the flavour's own threshold pair; the scenes use one threshold)
                m.TH_HIGH = s.th
            return self.frame.SearchByProjection(m, q, last_frame=s.flavour != R.FRUSTUM, occupied=s.occupied)
        finally:
            self.afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)

    def close(self):
        for o in (self.last, self.frame, self.points):
            if o is not None:
                o.close()


def fill_store(points, P):
    ids = np.flatnonzero(P.flags & R.SET).astype(np.int32)
    points.set(ids, pos=P.pos[ids], normal=P.normal[ids], min_distance=P.min_distance[ids], max_distance=P.max_distance[ids],
               ref_size=P.ref_size[ids], ref_distance=P.ref_distance[ids], ref_sigma=P.ref_sigma[ids])
    points.set_flags(ids, bad=P.flags[ids] & R.BAD, observed=P.flags[ids] & R.OBSERVED)
    points.set_descriptors(ids, P.descriptors[ids])


def assert_projection(got, want, name=""):
    assert np.array_equal(got["in_view"], want["in_view"]), name
    assert got["n_in_view"] == want["n_in_view"], name
    for k in FLOATS:
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (name, k, got[k], want[k])


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_constructed_scene_projection(afv, gpu_ctx, c):
    rig = Rig(afv, gpu_ctx, c)
    try:
        assert_projection(rig.project(), c.project(), c.name)
    finally:
        rig.close()


@pytest.mark.parametrize("seed,fl", RANDOM, ids=["seed%d_flavour%d" % sf for sf in RANDOM])
def test_random_scene_projection_and_search(afv, gpu_ctx, seed, fl):
    s = random_scene(seed, fl)
    rig = Rig(afv, gpu_ctx, s)
    try:
        assert_projection(rig.project(), s.project(), s.name)
        check_search(afv, rig, s)
    finally:
        rig.close()


def check_search(afv, rig, s, ids=None):
    if ids is not None:
        s = S.Scene(s.name, None, s.flavour, s.P, s.cam, ids, None, radius_th=s.radius_th, radius_scale=s.radius_scale, cos_limit=s.cos_limit,
                    last_sizes=None if s.last_sizes is None else s.last_sizes[:len(ids)],
                    last_angles=None if s.last_angles is None else s.last_angles[:len(ids)], feat=s.feat, th=s.th, nnratio=s.nnratio,
                    check_orientation=s.check_orientation, occupied=s.occupied, inf_gate=s.inf_gate)
    want, wn, o = S.expected_search(afv, PR, s)
    got, n, in_view = rig.search(s.ids)
    assert n == wn and np.array_equal(got, want), s.name
    if in_view is not None:
        assert np.array_equal(in_view, o["in_view"]), s.name
    if s.flavour == R.RELOC and s.last_angles is not None:
        got, n, _ = rig.search(s.ids, host_angles=True)
        assert n == wn and np.array_equal(got, want), s.name
    Q, _ = s.queries()
    if len(s.ids):
        host, hn = rig.host_array_search(Q)
        assert hn == wn and np.array_equal(host, want), s.name
    return wn


@pytest.mark.parametrize("engine", [1, 3, 0, 2], ids=["fixed_point_one_launch", "fixed_point_two_launches", "ordered_walk", "default"])
@pytest.mark.parametrize("c", SEARCH, ids=[c.name for c in SEARCH])
def test_constructed_scene_search(afv, gpu_ctx, c, engine):
    gpu_ctx.check(gpu_ctx.lib.afv_set_projection_resolve(gpu_ctx.handle, engine), "afv_set_projection_resolve")
    rig = Rig(afv, gpu_ctx, c)
    try:
        assert check_search(afv, rig, c) >= 1
    finally:
        rig.close()
        gpu_ctx.check(gpu_ctx.lib.afv_set_projection_resolve(gpu_ctx.handle, 2), "afv_set_projection_resolve")


@pytest.mark.parametrize("engine", [1, 3, 0], ids=["fixed_point_one_launch", "fixed_point_two_launches", "ordered_walk"])
def test_random_scene_search_on_every_engine(afv, gpu_ctx, engine):
    gpu_ctx.check(gpu_ctx.lib.afv_set_projection_resolve(gpu_ctx.handle, engine), "afv_set_projection_resolve")
    rigs = []
    try:
        for fl in (R.FRUSTUM, R.LASTFRAME, R.FUSE):
            s = random_scene(1, fl)
            rigs.append(Rig(afv, gpu_ctx, s))
            assert check_search(afv, rigs[-1], s) >= 5
    finally:
        for r in rigs:
            r.close()
        gpu_ctx.check(gpu_ctx.lib.afv_set_projection_resolve(gpu_ctx.handle, 2), "afv_set_projection_resolve")


def test_contested_feature_follows_the_id_order(afv, gpu_ctx):
    a, b = (next(c for c in CASES if c.name == n) for n in ("contest_order_01", "contest_order_10"))
    ra, rb = Rig(afv, gpu_ctx, a), Rig(afv, gpu_ctx, b)
    try:
        ga, gb = ra.search()[0], rb.search()[0]
        assert ga[0] == 0 and gb[0] == 0 and a.ids[ga[0]] == 0 and b.ids[gb[0]] == 1
    finally:
        ra.close(); rb.close()


def test_stereo_gates_and_the_chi_square_gate(afv, gpu_ctx):
    """the scenes whose answer hangs on q_ur / q_er under LASTFRAME and FUSE, and on keyPtsInf under FusePoints(use_inf_gate=True)"""
    want = {"er_sigma_gate": [0, -1], "stereo_gate_lastframe": [0, -1], "stereo_fuse_inf_gate": [0, 3, -1]}
    for name, answer in want.items():
        c = next(c for c in CASES if c.name == name)
        rig = Rig(afv, gpu_ctx, c)
        try:
            assert rig.search()[0].tolist() == answer, name
        finally:
            rig.close()


def test_another_size_tolerance(afv):
    """the size band is size / sizeTolerance .. size * sizeTolerance of the FRAME: a context whose scale factor is 1.5"""
    ctx = afv.Context(nlevels=4, scale_factor=1.5)
    s0 = random_scene(0, R.FRUSTUM)
    cam = R.Camera(Rcw=s0.cam.Rcw, tcw=s0.cam.tcw, Ow=s0.cam.Ow, mbf=8.0, tol=1.5)
    s = S.Scene("tol_1.5", None, R.FRUSTUM, s0.P, cam, s0.ids, None, radius_th=s0.radius_th, feat=s0.feat)
    rig = Rig(afv, ctx, s)
    try:
        got, want = rig.project(), s.project()
        assert_projection(got, want, s.name)
        assert not np.array_equal(want["qmax"], s0.project()["qmax"])
        assert check_search(afv, rig, s) >= 5
    finally:
        rig.close()
        ctx.close()


@pytest.mark.parametrize("nq", [0, 1, 63, 64, 65, 257])
def test_wavefront_and_workgroup_edges(afv, gpu_ctx, nq):
    """a thread per query in 256-thread workgroups: the counts at which a wavefront / a workgroup fills up; ids in shuffled order, capacity 512"""
    for fl in (R.FRUSTUM, R.LASTFRAME, R.FUSE):
        s = random_scene(2, fl)
        assert s.P.capacity == 512
        ids = s.ids[:nq]
        rig = Rig(afv, gpu_ctx, s)
        try:
            want = R.project(s.P, s.cam, ids, fl, **dict(s.kw(), last_sizes=None if s.last_sizes is None else s.last_sizes[:nq]))
            assert_projection(rig.project(ids), want, "%s nq=%d" % (s.name, nq))
            check_search(afv, rig, s, ids)
        finally:
            rig.close()


def _with_rows(s, desc_bytes, float_dim, seed=9):
    """the scene's geometry with descriptor rows of another kind: (Points, Features)"""
    rs = np.random.RandomState(seed)
    P0 = s.P
    P = R.Points(P0.capacity, desc_bytes, float_dim)
    for k in ("pos", "normal", "min_distance", "max_distance", "ref_size", "ref_distance", "ref_sigma", "flags"):
        getattr(P, k)[:] = getattr(P0, k)
    if float_dim:
        P.descriptors[:] = rs.uniform(0, 4, P.descriptors.shape)
    else:
        P.descriptors[:] = rs.randint(0, 256, P.descriptors.shape)
    o = s.project()
    f0 = s.feat
    desc = (rs.uniform(0, 4, (f0.n, float_dim)).astype(np.float32) if float_dim else rs.randint(0, 256, (f0.n, desc_bytes)).astype(np.uint8))
    keep = np.flatnonzero(o["in_view"])[:100]          # the order random_scene placed the features in
    for k, q in enumerate(keep):
        if float_dim:
            desc[k] = P.descriptors[s.ids[q]] + rs.uniform(-0.05, 0.05, float_dim).astype(np.float32)
        else:
            desc[k] = P.descriptors[s.ids[q]]
            desc[k, rs.randint(0, desc_bytes)] ^= np.uint8(1 << rs.randint(0, 8))
    return P, S.Features(f0.x, f0.y, f0.sizes, desc, angles=f0.angles, u_right=f0.u_right)


@pytest.mark.parametrize("desc_bytes,float_dim", [(32, 0), (61, 0), (20, 0), (256, 64)], ids=["32_bytes", "61_bytes", "20_bytes", "64_floats"])
def test_row_widths_by_host_rows_and_from_a_table(afv, gpu_ctx, desc_bytes, float_dim):
    base = random_scene(1, R.FRUSTUM)
    P, feat = _with_rows(base, desc_bytes, float_dim)
    s = S.Scene(base.name, None, base.flavour, P, base.cam, base.ids, None, radius_th=base.radius_th, feat=feat, th=64.0)
    rig = Rig(afv, gpu_ctx, s, P=P, feat=feat)
    table = None
    try:
        n1 = check_search(afv, rig, s)
        assert n1 >= 5
        first = rig.search()
        set_ids = np.flatnonzero(P.flags & R.SET).astype(np.int32)
        assert np.array_equal(rig.points.get(set_ids)["descriptors"], P.descriptors[set_ids])
        # the same rows out of a keyframe table: wipe the store's rows, then copy them device to device
        cap = 160
        table = (afv.table.DescriptorTable(gpu_ctx, 2, cap, float_dim=float_dim) if float_dim
                 else afv.table.DescriptorTable(gpu_ctx, 2, cap, desc_bytes=desc_bytes))
        slots = (np.arange(len(set_ids)) % 2).astype(np.int32)
        idx = (np.arange(len(set_ids)) // 2).astype(np.int32)
        for sl in (0, 1):
            table.set(sl, P.descriptors[set_ids[slots == sl]])
        rig.points.set_descriptors(set_ids, np.zeros_like(P.descriptors[set_ids]))
        assert not rig.points.get(set_ids)["descriptors"].any()
        rig.points.set_descriptors_from_table(set_ids, table, slots, idx)
        assert np.array_equal(rig.points.get(set_ids)["descriptors"], P.descriptors[set_ids])
        again = rig.search()
        assert again[1] == first[1] and np.array_equal(again[0], first[0])
        # a table of another width or kind is refused, as is a reference outside it
        other = afv.table.DescriptorTable(gpu_ctx, 1, 8, desc_bytes=48)
        try:
            z = np.zeros(1, np.int32)
            with pytest.raises(afv._lib.AfvError) as e:
                rig.points.set_descriptors_from_table(set_ids[:1], other, z, z)
            assert e.value.code == afv._lib.EUNSUPPORTED
        finally:
            other.close()
        for bad_slot, bad_idx in ((2, 0), (0, cap), (-1, 0), (0, len(set_ids))):
            with pytest.raises(afv._lib.AfvError) as e:
                rig.points.set_descriptors_from_table(set_ids[:1], table, np.array([bad_slot], np.int32), np.array([bad_idx], np.int32))
            assert e.value.code == afv._lib.EINVAL
        assert np.array_equal(rig.points.get(set_ids)["descriptors"], P.descriptors[set_ids])   # nothing moved
    finally:
        if table is not None:
            table.close()
        rig.close()


def test_store_updated_between_two_searches(afv, gpu_ctx):
    s = S.random_scene(0, R.FRUSTUM)   # (a copy of its own: the store changes)
    rig = Rig(afv, gpu_ctx, s)
    try:
        n1 = check_search(afv, rig, s)
        before = rig.project()
        moved = np.flatnonzero(before["in_view"])[::3]
        ids = s.ids[moved]
        new_pos = s.P.pos[ids] + np.float32([0.3, -0.2, 0.1])
        # SetWorldPos alone: the other fields stay as they are, on both sides
        s.P.set(ids, pos=new_pos)
        rig.points.set(ids, pos=new_pos)
        s.P.set_flags(ids[:4], bad=np.ones(4))
        rig.points.set_flags(ids[:4], bad=np.ones(4))
        got = rig.points.get(ids)
        assert np.array_equal(got["pos"], s.P.pos[ids]) and np.array_equal(got["normal"], s.P.normal[ids])
        assert np.array_equal(got["ref_size"], s.P.ref_size[ids]) and np.array_equal(got["flags"], s.P.flags[ids])
        after = rig.project()
        assert_projection(after, s.project(), "after the update")
        assert not np.array_equal(after["u"], before["u"]) and not after["in_view"][moved[:4]].any()
        n2 = check_search(afv, rig, s)
        assert n1 >= 5 and n2 >= 5
    finally:
        rig.close()


def test_setters_leave_null_fields_and_refuse_bad_ids(afv, gpu_ctx):
    pts = afv.MapPoints(gpu_ctx, 16)
    try:
        ids = np.array([3, 9, 15], np.int32)
        pts.set(ids, pos=np.arange(9), ref_size=[1, 2, 3])
        pts.set(ids[:2], normal=np.ones((2, 3)), min_distance=[5, 6])
        pts.set_flags(ids[1:], observed=[1, 1])
        g = pts.get(np.array([3, 9, 15, 0], np.int32))
        assert g["pos"].tolist() == [[0, 1, 2], [3, 4, 5], [6, 7, 8], [0, 0, 0]]
        assert g["normal"].tolist() == [[1, 1, 1], [1, 1, 1], [0, 0, 0], [0, 0, 0]]
        assert g["ref_size"].tolist() == [1, 2, 3, 0] and g["min_distance"].tolist() == [5, 6, 0, 0]
        assert g["flags"].tolist() == [R.SET, R.SET | R.OBSERVED, R.SET | R.OBSERVED, 0]
        for bad in ([16], [-1], [3, 99]):
            with pytest.raises(afv._lib.AfvError) as e:
                pts.set(np.array(bad, np.int32), ref_size=np.full(len(bad), 7.0))
            assert e.value.code == afv._lib.EINVAL
        assert pts.get(ids)["ref_size"].tolist() == [1, 2, 3]     # the refused call wrote nothing
        for cap in (0, -1, (1 << 22) + 1):
            with pytest.raises(afv._lib.AfvError) as e:
                afv.MapPoints(gpu_ctx, cap)
            assert e.value.code == afv._lib.EINVAL
    finally:
        pts.close()


def test_refusals_before_any_launch(afv, gpu_ctx):
    L = afv._lib
    s = next(c for c in CASES if c.name == "lastframe_search")
    rig = Rig(afv, gpu_ctx, s)
    other_ctx = afv.Context()
    try:
        f, lib = rig.frame, gpu_ctx.lib
        n = f.N
        out = np.full(max(n, 1), -1, np.int32); nm = np.zeros(1, np.int32)

        def call(edit, frame=f):
            rec, keep = f._point_search(rig.points, s.ids, R.LASTFRAME, 7.0, th=64.0, nnratio=0.9, qframe=rig.last)
            edit(rec)
            return lib.afv_frame_search_points(frame.handle, C.byref(rec), L.ptr(out), L.ptr(nm), None, None)

        assert call(lambda r: None) == L.OK
        assert call(lambda r: setattr(r, "qframe", None)) == L.EINVAL                  # LASTFRAME without its last frame
        assert call(lambda r: setattr(r, "struct_size", 8)) == L.EINVAL
        assert call(lambda r: setattr(r, "struct_size", 5 * C.sizeof(L.PointSearch))) == L.EINVAL
        assert call(lambda r: setattr(r, "flavour", R.FUSE)) == L.EINVAL               # Fuse has its own entry point
        assert call(lambda r: setattr(r, "flavour", 7)) == L.EINVAL
        assert call(lambda r: setattr(r, "nq", 65536)) == L.EINVAL
        big = np.array([0, 64], np.int32)                                              # an id at the capacity
        assert call(lambda r: (setattr(r, "ids", L.ptr(big)), setattr(r, "nq", 2))) == L.EINVAL
        # a store on another context; a store of another width; a frame without a pose
        foreign = afv.MapPoints(other_ctx, 64)
        assert call(lambda r: setattr(r, "points", foreign.handle)) == L.EINVAL
        foreign.close()
        wide = afv.MapPoints(gpu_ctx, 64, desc_bytes=61)
        assert call(lambda r: setattr(r, "points", wide.handle)) == L.EUNSUPPORTED
        wide.close()
        fl = afv.MapPoints(gpu_ctx, 64, float_dim=64)
        assert call(lambda r: setattr(r, "points", fl.handle)) == L.EUNSUPPORTED
        fl.close()
        bare = afv.Frame(gpu_ctx, max_x=S.W, max_y=S.H, cap=4)
        bare.set_features(np.zeros(1, afv.KP_DTYPE), np.zeros((1, 32), np.uint8))
        assert call(lambda r: None, frame=bare) == L.EINVAL
        bare.close()
        # a frame in the query role that the flavour does not read is ignored, however short or stale it is
        short = afv.Frame(gpu_ctx, max_x=S.W, max_y=S.H, cap=4)
        short.set_features(np.zeros(1, afv.KP_DTYPE), np.zeros((1, 32), np.uint8))
        assert call(lambda r: (setattr(r, "flavour", R.FRUSTUM), setattr(r, "qframe", short.handle))) == L.OK
        assert call(lambda r: setattr(r, "qframe", short.handle)) == L.EINVAL             # LASTFRAME reads it: too short
        stale = short.handle.value
        short.close()
        assert call(lambda r: (setattr(r, "flavour", R.FRUSTUM), setattr(r, "qframe", stale))) == L.OK
        assert call(lambda r: setattr(r, "qframe", stale)) == L.EINVAL                    # ... and a destroyed one is refused, not read
        # nq == 0 is legal
        assert call(lambda r: setattr(r, "nq", 0)) == L.OK and nm[0] == 0 and (out[:n] == -1).all()
        best = np.zeros(8, np.int32)
        rec, keep = f._point_search(rig.points, s.ids, R.FRUSTUM, 7.0, th=64.0)
        assert lib.afv_frame_fuse_points(f.handle, C.byref(rec), 0, L.ptr(best), L.ptr(nm)) == L.EINVAL   # not the Fuse flavour
    finally:
        other_ctx.close()
        rig.close()
