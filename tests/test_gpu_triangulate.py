"""-m gpu: afv_table_set_scale / afv_table_triangulate and DescriptorTable.CreateNewMapPoints against the restatement tests/_tri_ref.py on
the constructed and the seeded random scenes of tests/_tri_scenes.py - status, route, new_id and n_new exactly, x3D and every field of the
store as bits.  tests/test_tri_ref_cpu.py proves on the CPU that every constructed scene reaches the comparison it is named after."""
import ctypes as C

import numpy as np
import pytest

import _tri_ref as R
import _tri_scenes as S

pytestmark = pytest.mark.gpu
CAP = 320
FIELDS = ("pos", "normal", "min_distance", "max_distance", "ref_size", "ref_distance", "ref_sigma")
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rows_for(n, seed, desc_bytes=32, float_dim=0):
    rng = np.random.default_rng(500 + seed)
    return rng.normal(0, 1, (n, float_dim)).astype(np.float32) if float_dim else rng.integers(0, 256, (n, desc_bytes), dtype=np.uint8)


def make_table(afv, ctx, nsets, desc_bytes=32, float_dim=0):
    return afv.table.DescriptorTable(ctx, nsets, CAP, **({"float_dim": float_dim} if float_dim else {"desc_bytes": desc_bytes}))


def fill_slot(table, slot, kf, rows, scale=True, featvec=False):
    table.set(slot, rows)
    table.set_geometry(slot, kf.x, kf.y, kf.sigma2, u_right=kf.u_right)
    if scale:
        table.set_scale(slot, kf.size, kf.depth, kf.x_dist, kf.y_dist)
    if featvec:   # one node that holds every feature in index order: the restatement's "no vocabulary"
        table.set_featvec(slot, [0], [0, kf.n], np.arange(kf.n))


def c_jobs(afv, jobs):
    arr = (afv._lib.TriPointsJob * len(jobs))()
    for j, src in zip(arr, jobs):
        j.struct_size = C.sizeof(afv._lib.TriPointsJob)
        for name in ("Rcw1", "tcw1", "Ow1", "Rcw2", "tcw2", "Ow2"):
            dst, v = getattr(j, name), getattr(src, name)
            for k in range(len(v)):
                dst[k] = v[k]
        for name in R.Job.FIELDS:
            setattr(j, name, getattr(src, name))
    return arr


def pad(m):
    out = np.full((1, CAP), -1, np.int32)
    out[0, :len(m)] = m
    return out


def assert_outputs(got, want, name=""):
    status, route, x3d, new_id, n_new = got
    w_status, w_route, w_x3d, w_id, w_n = want[:5]
    assert np.array_equal(status, w_status), (name, "status")
    assert np.array_equal(route, w_route), (name, "route")
    assert np.array_equal(bits(x3d), bits(w_x3d)), (name, "x3d")
    assert np.array_equal(new_id, w_id) and np.array_equal(n_new, w_n), (name, "ids")


def assert_store(points, before, want_points, rows_of, name=""):
    """every new id holds the restatement's fields, flags set | observed and its descriptor row; every other id is as it was"""
    ids = np.arange(points.capacity, dtype=np.int32)
    after = points.get(ids)
    new = np.zeros(points.capacity, bool)
    for nid, p, i, f in want_points:
        new[nid] = True
        for k in FIELDS:
            assert np.array_equal(bits(after[k][nid]), bits(f[k])), (name, nid, k)
        assert after["flags"][nid] == f["flags"] == 5, (name, nid)
        assert after["descriptors"][nid].tobytes() == rows_of(p, i).tobytes(), (name, nid, "row")
    for k in after:
        assert after[k][~new].tobytes() == before[k][~new].tobytes(), (name, k, "an id that is not new changed")


def prefilled_store(afv, ctx, capacity, desc_bytes=32, float_dim=0):
    pts = afv.MapPoints(ctx, capacity, desc_bytes=desc_bytes, float_dim=float_dim)
    ids = np.arange(0, capacity, 3, dtype=np.int32)
    rng = np.random.default_rng(3)
    pts.set(ids, pos=rng.normal(0, 1, (len(ids), 3)), normal=rng.normal(0, 1, (len(ids), 3)), min_distance=rng.uniform(1, 2, len(ids)),
            max_distance=rng.uniform(3, 4, len(ids)), ref_size=np.ones(len(ids)), ref_distance=rng.uniform(1, 2, len(ids)), ref_sigma=np.ones(len(ids)))
    pts.set_descriptors(ids, rows_for(len(ids), 99, desc_bytes, float_dim))
    return pts, pts.get(np.arange(capacity, dtype=np.int32))


def test_constructed_scenes(afv, gpu_ctx):
    scenes = S.all_constructed()
    a, b, jobs, m = S.pack(scenes, CAP)
    assert len(scenes) <= 64
    P = len(scenes)
    want = cached("constructed", lambda: R.triangulate(jobs, [a] * P, [b] * P, m, first_id=5))
    ra, rb = rows_for(a.n, 1), rows_for(b.n, 2)
    t = make_table(afv, gpu_ctx, 2)
    pts, before = prefilled_store(afv, gpu_ctx, 64)
    try:
        fill_slot(t, 0, a, ra); fill_slot(t, 1, b, rb)
        got = t.triangulate([0] * P, [1] * P, c_jobs(afv, jobs), m, points=pts, first_id=5)
        for k, s in enumerate(scenes):   # a failure names its scene
            assert (got[0][k, k], got[1][k, k]) == (s.status, s.route), (s.name, s.on)
        assert_outputs(got, want, "constructed")
        assert_store(pts, before, want[5], lambda p, i: ra[i], "constructed")
        no_store = t.triangulate([0] * P, [1] * P, c_jobs(afv, jobs), m, first_id=5)   # the same call without a store
        assert_outputs(no_store, want, "constructed, no store")
    finally:
        pts.close(); t.close()


ROWS = {"mono": (32, 0), "a_stereo": (61, 0), "b_stereo": (0, 128), "both_stereo": (32, 0)}


@pytest.mark.parametrize("seed", S.SEEDS)
@pytest.mark.parametrize("kind", S.KINDS)
def test_random_scenes(afv, gpu_ctx, kind, seed):
    """rows: binary of 32 bytes, of 61 bytes (a_stereo) and float of 128 (b_stereo)"""
    job, a, b, m = S.random_scene(kind, seed)
    m = pad(m)
    want = cached(("random", kind, seed), lambda: R.triangulate([job], [a], [b], m, first_id=11))
    db, fd = ROWS[kind]
    ra, rb = rows_for(a.n, 1, db, fd), rows_for(b.n, 2, db, fd)
    t = make_table(afv, gpu_ctx, 2, db, fd)
    pts, before = prefilled_store(afv, gpu_ctx, 80, db or 32, fd)
    try:
        fill_slot(t, 0, a, ra); fill_slot(t, 1, b, rb)
        got = t.triangulate([0], [1], c_jobs(afv, [job]), m, points=pts, first_id=11)
        assert_outputs(got, want, (kind, seed))
        assert_store(pts, before, want[5], lambda p, i: ra[i], (kind, seed))
    finally:
        pts.close(); t.close()


def test_match_counts_at_the_lane_wavefront_and_workgroup_edges(afv, gpu_ctx):
    """0, 1, 63, 64, 65, 256 and 257 matches over a keyframe of 320 features: seven pairs of one call"""
    job, a, b, m = cached("big", lambda: S.random_scene("both_stereo", 5, n=CAP))
    counts = (0, 1, 63, 64, 65, 256, 257)
    rows = []
    for c in counts:
        keep = np.nonzero(m >= 0)[0][:c]
        assert len(keep) == c
        r = np.full(CAP, -1, np.int32)
        r[keep] = m[keep]
        rows.append(r)
    mm = np.stack(rows)
    P = len(counts)
    want = cached("edges", lambda: R.triangulate([job] * P, [a] * P, [b] * P, mm, first_id=0))
    assert want[4][0] == 0 and want[4][-1] > 128
    ra, rb = rows_for(a.n, 1), rows_for(b.n, 2)
    t = make_table(afv, gpu_ctx, 2)
    pts, before = prefilled_store(afv, gpu_ctx, 1024)
    try:
        fill_slot(t, 0, a, ra); fill_slot(t, 1, b, rb)
        got = t.triangulate([0] * P, [1] * P, c_jobs(afv, [job] * P), mm, points=pts)
        assert_outputs(got, want, "edges")
        assert_store(pts, before, want[5], lambda p, i: ra[i], "edges")
    finally:
        pts.close(); t.close()


@pytest.fixture(scope="module")
def world20():
    W = S.World(3, nn=20, n=40)
    none = np.zeros(W.n, np.uint8)
    m = np.full((20, CAP), -1, np.int32)
    for k in range(20):
        m[k, :W.n] = W.search(60.0)(k, none, none)
    return W, m


@pytest.mark.parametrize("npairs", [1, 7, 20])
def test_batches_equal_the_pairs_one_by_one(afv, gpu_ctx, world20, npairs):
    W, m = world20
    m = m[:npairs]
    want = cached(("batch", npairs), lambda: R.triangulate(W.jobs[:npairs], [W.kfs[0]] * npairs, W.kfs[1:npairs + 1], m, first_id=2))
    t = make_table(afv, gpu_ctx, 21)
    pts, before = prefilled_store(afv, gpu_ctx, 900)
    single, _ = prefilled_store(afv, gpu_ctx, 900)
    try:
        for k in range(npairs + 1):
            fill_slot(t, k, W.kfs[k], W.desc[k])
        pa, pb = [0] * npairs, list(range(1, npairs + 1))
        jobs = c_jobs(afv, W.jobs[:npairs])
        got = t.triangulate(pa, pb, jobs, m, points=pts, first_id=2)
        assert_outputs(got, want, npairs)
        assert_store(pts, before, want[5], lambda p, i: W.desc[0][i], npairs)
        nid = 2
        for p in range(npairs):   # the same pairs called one by one, ids offset accordingly
            one = t.triangulate([0], [pb[p]], c_jobs(afv, [W.jobs[p]]), m[p:p + 1], points=single, first_id=nid)
            assert_outputs(one, [w[p:p + 1] for w in want[:5]], (npairs, p))
            nid += int(one[4][0])
        ids = np.arange(900, dtype=np.int32)
        a, b = pts.get(ids), single.get(ids)
        assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    finally:
        pts.close(); single.close(); t.close()


def test_a_slot_filled_from_a_frame(afv, gpu_ctx):
    """sizes, depth and the distorted keypoints arrive from the frame (afv_table_set_from_frame), device to device"""
    job, a, b, m = S.random_scene("a_stereo", 1)
    rng = np.random.default_rng(8)
    kps = np.zeros(a.n, afv.KP_DTYPE)
    kps["x"], kps["y"] = a.x + rng.normal(0, 0.4, a.n).astype(np.float32), a.y + rng.normal(0, 0.4, a.n).astype(np.float32)   # mvKeys, distorted
    depth_img = rng.uniform(2.0, 9.0, (480, 640)).astype(np.float32)
    depth_img[::7, ::5] = 0.0                                                                                                 # no depth there
    ra, rb = rows_for(a.n, 1), rows_for(b.n, 2)
    fr = afv.Frame(gpu_ctx, max_x=640.0, max_y=480.0, distorted=True, cap=CAP)
    t = make_table(afv, gpu_ctx, 2)
    pts, before = prefilled_store(afv, gpu_ctx, 80)
    try:
        fr.set_features(kps, ra, sizes=a.size)
        fr.set_undistorted(a.x, a.y)
        fr.ComputeStereoFromRGBD(depth_img, float(job.mbf1))
        ur, dp, _, _ = fr.stereo()
        assert (dp > 0).sum() > a.n // 2 and (dp < 0).sum() > 0
        a2 = R.KF(a.x, a.y, a.size * a.size, a.size, u_right=ur, depth=dp, x_dist=kps["x"], y_dist=kps["y"])   # keyPtsSigma2 = size^2
        t.set_from_frame(0, fr)
        fill_slot(t, 1, b, rb)
        want = R.triangulate([job], [a2], [b], pad(m), first_id=0)
        assert {1, 0} <= set(want[1][0][want[0][0] > 0].tolist())     # both the unprojection from a and the triangulation are taken
        got = t.triangulate([0], [1], c_jobs(afv, [job]), pad(m), points=pts)
        assert_outputs(got, want, "from frame")
        assert_store(pts, before, want[5], lambda p, i: ra[i], "from frame")
    finally:
        pts.close(); t.close(); fr.close()


def test_a_cloned_table_answers_as_its_source(afv, gpu_ctx):
    job, a, b, m = S.random_scene("both_stereo", 2)
    want = cached(("random", "both_stereo", 2, 0), lambda: R.triangulate([job], [a], [b], pad(m), first_id=0))
    src, dst = make_table(afv, gpu_ctx, 2), make_table(afv, gpu_ctx, 2)
    try:
        fill_slot(src, 0, a, rows_for(a.n, 1)); fill_slot(src, 1, b, rows_for(b.n, 2))
        src.clone_into(dst)
        assert_outputs(dst.triangulate([0], [1], c_jobs(afv, [job]), pad(m)), want, "clone")
        src.set(1, rows_for(b.n, 2))        # a recycled slot forgets its planes; the clone keeps its own
        with pytest.raises(afv._lib.AfvError) as e:
            src.triangulate([0], [1], c_jobs(afv, [job]), pad(m))
        assert e.value.code == afv._lib.EINVAL
        assert_outputs(dst.triangulate([0], [1], c_jobs(afv, [job]), pad(m)), want, "clone, after the source moved on")
    finally:
        src.close(); dst.close()


def test_error_answers(afv, gpu_ctx):
    L = afv._lib
    job, a, b, m = S.random_scene("mono", 0)
    ra, rb = rows_for(a.n, 1), rows_for(b.n, 2)
    t = make_table(afv, gpu_ctx, 3)
    pts, before = prefilled_store(afv, gpu_ctx, 20)
    other_width, other_kind = afv.MapPoints(gpu_ctx, 64, desc_bytes=61), afv.MapPoints(gpu_ctx, 64, float_dim=8)
    jobs = c_jobs(afv, [job])

    def code(fn):
        with pytest.raises(L.AfvError) as e:
            fn()
        return e.value.code
    try:
        fill_slot(t, 0, a, ra); fill_slot(t, 1, b, rb)
        fill_slot(t, 2, b, rb, scale=False)
        assert code(lambda: t.triangulate([0], [2], jobs, pad(m))) == L.EINVAL                      # a slot without its scale planes
        assert code(lambda: t.set_scale(2, b.size[:b.n], x_dist=b.x)) == L.EINVAL                    # x_dist without y_dist
        bad = pad(m); bad[0, 3] = b.n
        assert code(lambda: t.triangulate([0], [1], jobs, bad)) == L.EINVAL                          # match12 out of range
        bad = pad(m); bad[0, 3] = -2
        assert code(lambda: t.triangulate([0], [1], jobs, bad)) == L.EINVAL
        bad = pad(m); bad[0, a.n] = 0
        assert code(lambda: t.triangulate([0], [1], jobs, bad)) == L.EINVAL                          # a match at a feature a does not have
        want = R.triangulate([job], [a], [b], pad(m), first_id=0)
        assert want[4][0] > 20
        first = 20 - int(want[4][0]) + 1                                                             # one id too many
        status = np.full((1, CAP), 77, np.uint8)
        rc = L.load().afv_table_triangulate(t.handle, L.ptr(np.zeros(1, np.int32)), L.ptr(np.ones(1, np.int32)), jobs, 1, L.ptr(pad(m)), pts.handle,
                                            max(first, 0), L.ptr(status), None, None, None, None)
        assert rc == L.ECAPACITY and np.all(status == 77)                                            # capacity exceeded: outputs untouched
        after = pts.get(np.arange(20, dtype=np.int32))
        assert all(after[k].tobytes() == before[k].tobytes() for k in after)                         # ... and so is the store
        assert code(lambda: t.triangulate([0], [1], jobs, pad(m), points=other_width)) == L.EUNSUPPORTED
        assert code(lambda: t.triangulate([0], [1], jobs, pad(m), points=other_kind)) == L.EUNSUPPORTED
        assert code(lambda: t.triangulate([0], [5], jobs, pad(m))) == L.EINVAL                        # a slot out of range
        jobs[0].struct_size = 6
        assert code(lambda: t.triangulate([0], [1], jobs, pad(m))) == L.EINVAL                        # an unknown struct_size
    finally:
        pts.close(); other_width.close(); other_kind.close(); t.close()


@pytest.fixture(scope="module")
def world3():
    W = S.World(1, nn=3, n=40)
    none = lambda: [np.zeros(W.n, np.uint8) for _ in range(W.nn)]
    return W, R.create_new_map_points(W.kfs[0], W.kfs[1:], W.jobs, W.search(60.0), np.zeros(W.n, np.uint8), none(), first_id=4)


def run_chain(afv, ctx, W, pts):
    t = make_table(afv, ctx, 4)
    for k in range(4):
        fill_slot(t, k, W.kfs[k], W.desc[k], featvec=True)
    has_mp = {k: np.zeros(W.n, np.uint8) for k in range(4)}
    cams = {k: W.cams[k] for k in range(4)}
    return t, t.CreateNewMapPoints(pts, 0, [1, 2, 3], cams, np.stack(W.F12), np.stack(W.epipoles), 60.0, has_mp, 4), has_mp


def test_create_new_map_points_against_the_composed_restatement(afv, gpu_ctx, world3):
    W, want = world3
    pts, before = prefilled_store(afv, gpu_ctx, 200)
    t = None
    try:
        t, got, has_mp = run_chain(afv, gpu_ctx, W, pts)
        assert [(nid, [(0, i), (k + 1, j)]) for nid, k, i, j, _ in want] == got
        assert len(got) > W.n // 2 and len({obs[0][1] for _, obs in got}) == len(got)      # a feature of the current keyframe: at most one point
        assert int(has_mp[0].sum()) == len(got)
        assert_store(pts, before, [(nid, k, i, f) for nid, k, i, j, f in want], lambda p, i: W.desc[0][i], "chain")
    finally:
        pts.close()
        if t is not None:
            t.close()


def test_search_local_points_sees_the_new_points_without_an_upload(afv, gpu_ctx, world3):
    """Frame.SearchLocalPoints on the ids just created, against the same search on a store filled with afv_points_set from the restatement"""
    W, want = world3
    made, _ = prefilled_store(afv, gpu_ctx, 200)
    host, _ = prefilled_store(afv, gpu_ctx, 200)
    fr = afv.Frame(gpu_ctx, max_x=640.0, max_y=480.0, cap=CAP)
    t = None
    try:
        t, got, _ = run_chain(afv, gpu_ctx, W, made)
        ids = np.array([nid for nid, _ in got], np.int32)
        f = [w[4] for w in want]
        host.set(ids, **{k: np.stack([x[k] for x in f]) for k in FIELDS})
        host.set_flags(ids, bad=np.zeros(len(ids)), observed=np.ones(len(ids)))
        host.set_descriptors(ids, np.stack([W.desc[0][i] for _, _, i, _, _ in want]))
        kf, cam = W.kfs[2], W.cams[2]
        kps = np.zeros(kf.n, afv.KP_DTYPE)
        kps["x"], kps["y"] = kf.x, kf.y
        fr.set_features(kps, W.desc[2], sizes=kf.size)
        fr.set_pose(cam["Rcw"], cam["tcw"], cam["Ow"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], 0.0)
        afv.FeatureMatcher.setDescriptorDistanceThresholds(100.0)
        try:
            m = afv.FeatureMatcher(0.8, False, ctx=gpu_ctx)
            a = fr.SearchLocalPoints(m, made, ids, 3.0)
            b = fr.SearchLocalPoints(m, host, ids, 3.0)
        finally:
            afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)
        assert a[1] == b[1] and a[1] > len(ids) // 2
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    finally:
        made.close(); host.close(); fr.close()
        if t is not None:
            t.close()
