"""-m gpu: the duels of tests/_l2_scenes.py through every device route that evaluates the float L2^2, against the normative restatement:
match vectors, counts and - where a call returns them - the distance bits themselves, all as equalities.  tests/test_l2_scenes_cpu.py
proves on the CPU that each scene's expected outcome changes under the wrong arithmetic it is named after, so a route that passes here
does the differences in float, the squares in double, the groups of four, one running double in index order, and one rounding.

Which text of the library each test reaches:
  match_l2, dims 64 / 128            l2_topk_body via k_l2_topk<64|128> (k_match_l2.hip), k_l2_merge, k_l2_resolve
  match_l2, dims 100 / 7             l2sqr (k_tri_row.h) in the generic kernel of k_match.hip; 7 floats: its remainder loop
  table pairs, dims 64 / 128         l2_topk_body via k_l2_topk_pairs<64|128>; also through match_l2_pairs_device on the table's view
  table pairs, dim 256               k_l2_topk_pairs_split<256>: the running double parked in LDS between two parts
  table pairs, dims 36 / 200 / 1024  k_l2_topk_pairs_split<0>: one ragged part / two parts, ragged last / eight parts and 8-column chunks
  rescan                             l2_exact in k_l2_resolve (match_l2) and in k_l2_resolve_pairs (table, 64 and 256 floats)
  bow                                l2sqr (k_tri_row.h) in the BoW-guided kernels and in tri_row, from host views and from table slots
  projection                         proj_l2sqr (k_project.hip), its five call sites by the function they stand in:
                                       topk_query        every SearchByProjection / SearchForInitialization case, under both engines
                                       proj_resolve      the "used-up" local-map and last-frame cases under the ordered walk
                                       proj_resolve_wg   the same cases under the fixed point
                                       init_resolve      the "used-up" SearchForInitialization case (float jobs take its ordered walk)
                                       fuse_query        the Fuse cases
                                     Float jobs always go through the batch kernels: choose_route (afv_project.hip) gives neither the
                                     zero-copy inputs nor the one-launch ticket to a job with float rows, so the one-job kernels
                                     (k_proj_topk1, k_proj_resolve_wg1, k_match_fuse1, k_proj_search1) never see one, and the settings
                                     1 and 3 of afv_set_projection_resolve are the same route here: one of them is run.  Host arrays,
                                     resident frames and a float point store (afv_frame_search_points) differ in where the rows come from
  stereo                             stereo_l2sqr (k_stereo.hip)
  distinctive                        l2sqr (k_tri_row.h) in the median kernels of k_match.hip (host rows of any width: 7 floats reach the
                                     remainder loop; 67 rows: the path that does not stage the N x N distances in LDS) and in
                                     k_refresh.hip (table rows)
  refusals                           the argument checks that keep a dim % 4 remainder out of every other route (_l2_scenes.REFUSES_TAIL)
A test walks many scenes and reports the names of ALL that differ."""
import numpy as np
import pytest

import _l2_scenes as L

pytestmark = pytest.mark.gpu


def differing(scenes, run):
    bad = []
    for s in scenes:
        got = run(s)
        if not L.same(got, s.expected):
            bad.append((s.name, s.duel.how))
    return bad


@pytest.fixture(scope="module")
def matcher(afv, gpu_ctx):
    return afv.FeatureMatcher(1.0, False, ctx=gpu_ctx)


@pytest.fixture()
def thresholds_restored(afv, matcher):
    FM = afv.FeatureMatcher
    names = ("TH_LOW", "TH_HIGH", "descDistTh_low_reloc", "descDistTh_high_reloc")
    before = [getattr(FM, n) for n in names] + [matcher.mfNNratio, matcher.mbCheckOrientation]
    yield
    for n, v in zip(names, before):
        setattr(FM, n, v)
    matcher.mfNNratio, matcher.mbCheckOrientation = before[4], before[5]


def _match_l2(matcher, s):
    i = s.inputs
    got, n = matcher.match_l2(i["d1"], i["d2"], L.TH, 1.0, i.get("valid1"), i.get("valid2"))
    return got, np.int32(n)


@pytest.mark.parametrize("route", ["match_tiled", "match_generic"])
def test_match_l2(matcher, route):
    """the tiled kernels (64 / 128 floats; 65 x 67: two row tiles, three column chunks; with and without validity masks) and the generic
    kernel (100 floats, and 7: the remainder loop)"""
    scenes = L.scenes(route)
    assert {s.dim for s in scenes} == set(L.ROUTES[route])
    assert differing(scenes, lambda s: _match_l2(matcher, s)) == []


@pytest.mark.parametrize("dim", L.ROUTES["match_pairs"])
def test_table_pairs(afv, gpu_ctx, matcher, dim):
    """DescriptorTable.match_pairs and match_pairs_device, one pair per wrong arithmetic plus an empty set on either side, cap 70; at 64 and
    128 floats match_l2_pairs_device on the table's own view as well"""
    import torch
    scenes = [s for s in L.scenes("match_pairs") if s.dim == dim]
    assert len(scenes) >= 5
    k = len(scenes)
    table = afv.table.DescriptorTable(gpu_ctx, 2 * k + 1, 70, float_dim=dim)
    try:
        for i, s in enumerate(scenes):
            table.set(2 * i, s.inputs["d1"])
            table.set(2 * i + 1, s.inputs["d2"])
        pa = np.array([2 * i for i in range(k)] + [2 * k, 0], np.int32)
        pb = np.array([2 * i + 1 for i in range(k)] + [1, 2 * k], np.int32)
        m, nm = table.match_pairs(pa, pb, L.TH, 1.0, False)
        dm, dn = table.match_pairs_device(torch.from_numpy(pa).cuda(), torch.from_numpy(pb).cuda(), L.TH, 1.0, False)
        torch.cuda.synchronize()
        results = {"match_pairs": (m, nm), "match_pairs_device": (dm.cpu().numpy(), dn.cpu().numpy())}
        if dim in (64, 128):
            d, _, n = table.device_views()
            rm, rn = matcher.match_l2_pairs_device(d, n, torch.from_numpy(pa).cuda(), torch.from_numpy(pb).cuda(), L.TH, 1.0)
            torch.cuda.synchronize()
            results["match_l2_pairs_device"] = (rm.cpu().numpy(), rn.cpu().numpy())
        bad = []
        for name, (gm, gn) in results.items():
            bad += [(name,) + b for b in differing(scenes, lambda s: (gm[scenes.index(s), :L.N1], np.int32(gn[scenes.index(s)])))]
            assert np.all(gm[k:] == -1) and np.all(gn[k:] == 0), name             # the pairs with the empty set
            assert np.all(gm[:k, L.N1:] == -1), name
        assert bad == []
    finally:
        table.close()


def test_rescan_in_both_resolve_kernels(afv, gpu_ctx, matcher):
    """a row whose four keys are taken by the four rows before it: l2_exact decides its duel.  k_l2_resolve through match_l2 (64 floats),
    k_l2_resolve_pairs through the table (64 and 256 floats)"""
    scenes = L.scenes("rescan")
    bad = differing([s for s in scenes if s.dim == 64], lambda s: _match_l2(matcher, s))
    for dim in L.ROUTES["rescan"]:
        mine = [s for s in scenes if s.dim == dim]
        assert len(mine) >= 5
        n1 = len(mine[0].inputs["d1"])
        table = afv.table.DescriptorTable(gpu_ctx, 2 * len(mine), 16, float_dim=dim)
        try:
            for i, s in enumerate(mine):
                table.set(2 * i, s.inputs["d1"])
                table.set(2 * i + 1, s.inputs["d2"])
            m, nm = table.match_pairs(np.arange(0, 2 * len(mine), 2, dtype=np.int32), np.arange(1, 2 * len(mine), 2, dtype=np.int32), L.TH, 1.0, False)
            bad += [("table",) + b for b in differing(mine, lambda s: (m[mine.index(s), :n1], np.int32(nm[mine.index(s)])))]
        finally:
            table.close()
    assert bad == []


def test_bow_guided_and_triangulation_host_views(afv, matcher, thresholds_restored):
    """FeatureMatcher.SearchByBoW (KF, KF) and (KF, F) and SearchForTriangulation on host FeatureViews: 8 and 64 floats, one node and the
    node shapes of tests/_match_scenes.py"""
    from test_gpu_match_scenes import run_host
    scenes = L.scenes("bow")
    assert {s.dim for s in scenes} == {8, 64}
    assert differing(scenes, lambda s: _as_ref(run_host(afv, matcher, s.inputs["case"]))) == []


def _as_ref(res):
    got, n = res
    return np.asarray(got, np.int32), int(n)


@pytest.mark.parametrize("dim", L.ROUTES["bow"])
def test_bow_guided_and_triangulation_table_slots(afv, gpu_ctx, dim):
    """DescriptorTable.match_bow, match_bow_frame (host frame view) and match_triangulation over two slots of a float table"""
    from test_gpu_match_scenes import _one_node
    scenes = [s for s in L.scenes("bow") if s.dim == dim]
    cap = max(max(s.inputs["case"].K1.N, s.inputs["case"].K2.N) for s in scenes)
    table = afv.table.DescriptorTable(gpu_ctx, 2, cap, float_dim=dim)

    def run(s):
        c = s.inputs["case"]
        K1, K2 = _one_node(afv, c.K1), _one_node(afv, c.K2)
        for slot, K in ((0, K1), (1, K2)):
            if c.kind == "kff" and slot == 1:
                continue
            table.set(slot, K.descriptors, K.angles)
            table.set_featvec(slot, *K.csr()[:3])
            table.set_valid(slot, None if c.kind == "tri" else K.valid)
            if c.kind == "tri":
                table.set_geometry(slot, K.pts[:, 0], K.pts[:, 1], K.sigma2 if K.sigma2 is not None else np.ones(K.N, np.float32), K.u_right)
        if c.kind == "kfkf":
            m, nm = table.match_bow([0], [1], c.kw["th_low"], c.kw["nnratio"], False)
            return m[0, :K1.N], int(nm[0])
        if c.kind == "kff":
            m, nm = table.match_bow_frame([0], K2, c.kw["th_low"], c.kw["nnratio"], False)
            return m[0], int(nm[0])
        m, nm = table.match_triangulation([0], [1], np.asarray(c.kw["F12"], np.float32)[None], np.asarray(c.kw["epipole"], np.float32)[None],
                                          c.kw["th_low"], [K1.valid], [K2.valid], False)
        return m[0, :K1.N], int(nm[0])
    try:
        assert differing(scenes, lambda s: _as_ref(run(s))) == []
    finally:
        table.close()


@pytest.fixture(params=[1, 0], ids=["fixed_point", "ordered_walk"])
def proj_engine(request, gpu_ctx):
    gpu_ctx.check(gpu_ctx.lib.afv_set_projection_resolve(gpu_ctx.handle, request.param), "afv_set_projection_resolve")
    yield request.param
    gpu_ctx.check(gpu_ctx.lib.afv_set_projection_resolve(gpu_ctx.handle, 2), "afv_set_projection_resolve")


def test_projection_searches(afv, gpu_ctx, proj_engine):
    """SearchByProjection (local map, last frame), Fuse and SearchForInitialization under the fixed point and the ordered walk of
    afv_set_projection_resolve: host arrays and, for the searches a resident frame expresses, the frame"""
    from test_gpu_proj_scenes import _host, _matcher, _resident
    scenes = [s for s in L.scenes("projection") if "case" in s.inputs]
    assert {s.dim for s in scenes} == {8, 64} and any(s.name.endswith("used-up") for s in scenes)
    bad = differing(scenes, lambda s: _as_i32(_host(afv, gpu_ctx, s.inputs["case"])))

    def resident(s):
        c = s.inputs["case"]
        fr = _resident(afv, gpu_ctx, c.F)
        assert fr is not None
        try:
            m = _matcher(afv, gpu_ctx, c)
            if c.kw.get("fuse"):
                return _as_i32(fr.Fuse(m, c.Q, use_inf_gate=False))
            return _as_i32(fr.SearchByProjection(m, c.Q, last_frame=c.kw.get("last_frame", False)))
        finally:
            afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)
            fr.close()
    bad += [("resident",) + b for b in differing([s for s in scenes if s.inputs["case"].kind == "proj"], resident)]
    assert bad == []


def test_search_local_points_over_a_float_point_store(afv, gpu_ctx):
    """afv_frame_search_points: the queries' rows come from a resident MapPoints store of 8 and of 64 floats"""
    from test_gpu_points import Rig
    scenes = [s for s in L.scenes("projection") if "scene" in s.inputs]
    assert {s.dim for s in scenes} == {8, 64}

    def run(s):
        rig = Rig(afv, gpu_ctx, s.inputs["scene"])
        try:
            got, n, in_view = rig.search()
            return np.asarray(got, np.int32), np.int32(n), np.asarray(in_view, bool)
        finally:
            rig.close()
    assert differing(scenes, run) == []


def _as_i32(res):
    got, n = res
    return np.asarray(got, np.int32), np.int32(n)


@pytest.fixture(scope="module")
def sctx(afv):
    import torch
    import _stereo_scenes as SS
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = afv.Context(nfeatures=300, nlevels=SS.NLEVELS, scale_factor=SS.SCALE, max_width=SS.WIDTH, max_height=SS.HEIGHT)
    yield c
    c.close()


def test_stereo_match_on_float_rows(afv, sctx):
    """Frame.ComputeStereoMatches: one image row, two right candidates inside the disparity window; the chosen right index, the SAD and the
    bits of u_right and depth"""
    from test_gpu_stereo import _frame

    def run(s):
        sc = s.inputs["scene"]
        left, right = _frame(afv, sctx, sc.L, sc.pyrL), _frame(afv, sctx, sc.R, sc.pyrR)
        try:
            left.ComputeStereoMatches(right, sc.mbf, sc.fx, th_high=sc.th_high, th_low=sc.th_low)
            ur, dp, sad, br = left.stereo()
            return ur, dp, np.asarray(sad, np.int32), np.asarray(br, np.int32)
        finally:
            left.close(); right.close()
    scenes = L.scenes("stereo")
    assert {s.dim for s in scenes} == {8, 64}
    assert differing(scenes, run) == []


def test_distinctive_descriptors_of_host_rows(afv, gpu_ctx):
    """afv_distinctive_descriptors_f32: 3, 4 and 5 observations, and 67 (the N x N distances do not fit the staged form); best index and
    the bits of the median.  Host rows may have any width: 7 floats reach the remainder loop of the kernel's own copy of l2sqr"""
    scenes = L.scenes("distinctive")
    assert {s.dim for s in scenes} == {36, 128, 7} and any(len(s.inputs["rows"]) > 64 for s in scenes)
    assert any(s.dim == 7 and s.wrong == "tail_first" for s in scenes)
    bad = []
    for dim in (36, 128, 7):
        mine = [s for s in scenes if s.dim == dim]
        best, med = afv.ComputeDistinctiveDescriptors(gpu_ctx, [s.inputs["rows"] for s in mine])
        assert med.dtype == np.float32
        bad += differing(mine, lambda s: (np.int32(best[mine.index(s)]), med[mine.index(s)]))
    assert bad == []


@pytest.mark.parametrize("dim", L.REFRESH_DIMS)
def test_refresh_points_on_float_tables(afv, gpu_ctx, dim):
    """afv_table_refresh_points, the descriptor part: one point per scene, its observations one per keyframe slot"""
    import _refresh_ref as R
    import _refresh_scenes as RS
    from test_gpu_refresh import Rig
    scenes = [s for s in L.scenes("distinctive") if s.dim == dim]
    nslots = max(len(s.inputs["rows"]) for s in scenes)
    sc = RS.Scene(("float", dim), nslots=nslots, cap=len(scenes), seed=5)
    for p, s in enumerate(scenes):
        rows = s.inputs["rows"]
        for slot in range(len(rows)):
            sc.set_row(slot, p, rows[slot])
        sc.point(p, [(slot, p) for slot in range(len(rows))], 0)
    first = np.cumsum([0] + [len(s.inputs["rows"]) for s in scenes])
    rig = Rig(afv, gpu_ctx, sc)
    try:
        status, best, med = rig.refresh(afv, True, False)
        assert np.all(status == R.DONE) and med.dtype == np.float32
        assert differing(scenes, lambda s: (np.int32(best[scenes.index(s)] - first[scenes.index(s)]), med[scenes.index(s)])) == []
        stored = rig.points.get(np.arange(len(scenes), dtype=np.int32))["descriptors"]
        for p, s in enumerate(scenes):
            assert stored[p].tobytes() == s.inputs["rows"][int(s.expected[0])].tobytes(), s.name
    finally:
        rig.close()


def test_the_routes_listed_without_a_remainder_refuse_seven_floats(afv, gpu_ctx, matcher):
    """_l2_scenes.REFUSES_TAIL names, per route, the argument check that keeps rows with a dim % 4 remainder out; here each check is met
    with rows of 7 floats.  A route that took them would need a tail_first scene instead of a line in that list"""
    import ctypes as C
    import torch
    lib, AfvError = afv._lib, afv._lib.AfvError
    rows = np.zeros((4, 7), np.float32)
    seen = set()

    def refused(code, call):
        with pytest.raises(AfvError) as e:
            call()
        assert e.value.code == code

    # match_tiled: no error, the launcher declines and the caller takes the generic kernel (the first test of the launcher, nothing is read)
    tiled = gpu_ctx.lib.afv_launch_match_l2_tiled
    tiled.restype = C.c_int
    one = C.c_float(1.0)
    assert tiled(None, 1, None, 1, 7, None, None, one, one, None, None, None, 1, 32, None) == 0
    got, n = matcher.match_l2(rows + 1, rows, L.TH, 1.0)          # ... and 7 floats are matched all the same
    assert n == 0 and np.all(got == -1)
    seen.add("match_tiled")
    # match_pairs and rescan: the pairs launcher, the table, the raw entry point
    pairs = gpu_ctx.lib.afv_launch_match_l2_pairs
    pairs.restype = C.c_int
    assert pairs(None, None, 70, 7, None, None, 1, 0, one, one, None, None, None, None, None) == 0
    h = C.c_void_p()
    assert gpu_ctx.lib.afv_table_create_f32(gpu_ctx.handle, 2, 8, 7, C.byref(h)) == lib.EINVAL and not h.value
    with pytest.raises(ValueError):
        afv.table.DescriptorTable(gpu_ctx, 2, 8, float_dim=7)
    z = torch.zeros(1, dtype=torch.int32, device="cuda")
    refused(lib.EUNSUPPORTED, lambda: matcher.match_l2_pairs_device(torch.zeros((1, 8, 7), device="cuda"), z, z, z, L.TH, 1.0))
    seen.update(("match_pairs", "rescan"))
    # bow: host views
    K = afv.FeatureView(rows, None, None, np.zeros(4, np.float32), np.zeros((4, 2), np.float32), np.ones(4, np.float32), None)
    refused(lib.EINVAL, lambda: matcher.SearchByBoW(K, K))
    refused(lib.EINVAL, lambda: matcher.SearchByBoW(K, K, frame=True))
    refused(lib.EINVAL, lambda: matcher.SearchForTriangulation(K, K, np.zeros(9, np.float32), (0.0, 0.0)))
    K8 = afv.FeatureView(np.zeros((4, 8), np.float32), None, None, np.zeros(4, np.float32), np.zeros((4, 2), np.float32), np.ones(4, np.float32), None)
    assert matcher.SearchByBoW(K8, K8)[0].shape == (4,)          # (the same call with 8 floats is taken: the width is what was refused)
    seen.add("bow")
    # projection: host arrays, a resident frame, a point store; stereo: the resident frame
    F = afv.FrameGridView(rows, np.full((4, 2), 100.0, np.float32), np.ones(4, np.float32), angles=np.zeros(4, np.float32))
    Q = afv.ProjectionQueries(rows, np.full(4, 100.0, np.float32), np.full(4, 100.0, np.float32), np.full(4, 5.0, np.float32),
                              np.full(4, 0.5, np.float32), np.full(4, 2.0, np.float32), angles=np.zeros(4, np.float32))
    refused(lib.EINVAL, lambda: matcher.SearchByProjection(F, Q))
    F8 = afv.FrameGridView(np.zeros((4, 8), np.float32), np.full((4, 2), 100.0, np.float32), np.ones(4, np.float32), angles=np.zeros(4, np.float32))
    Q.descriptors = np.zeros((4, 8), np.float32)
    assert matcher.SearchByProjection(F8, Q)[0].shape == (4,)
    Q.descriptors = rows
    refused(lib.EINVAL, lambda: matcher.Fuse(F, Q))
    refused(lib.EINVAL, lambda: afv.Frame(gpu_ctx, float_dim=7))
    refused(lib.EINVAL, lambda: afv.MapPoints(gpu_ctx, 4, float_dim=7))
    seen.update(("projection", "stereo"))
    assert seen == set(L.REFUSES_TAIL)
