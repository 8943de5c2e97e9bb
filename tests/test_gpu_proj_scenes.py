"""-m gpu: the constructed scenes of tests/_proj_scenes.py (exact edges of the geometric filters and decision rules, dependency chains, answers
behind the key lists, rotation-histogram edges), the size regimes and job batches (njobs = 2 / 7 / 33) through the projection kernels,
bit-exact against the oracle - on the three engines of afv_set_projection_resolve, through the host-array entry points and through
resident frames.  tests/test_proj_ref_cpu.py proves on the CPU that every scene reaches the branch it is named after."""
import ctypes as C

import numpy as np
import pytest

import _proj_scenes as PS

pytestmark = pytest.mark.gpu

CASES = PS.all_constructed()
REGIMES = PS.size_regimes()
EINVAL = -1


@pytest.fixture(autouse=True, params=[1, 3, 0], ids=["fixed_point_one_launch", "fixed_point_two_launches", "ordered_walk"])
def proj_engine(request, gpu_ctx):
    gpu_ctx.check(gpu_ctx.lib.afv_set_projection_resolve(gpu_ctx.handle, request.param), "afv_set_projection_resolve")
    yield request.param
    gpu_ctx.check(gpu_ctx.lib.afv_set_projection_resolve(gpu_ctx.handle, 2), "afv_set_projection_resolve")


def _oracle(oracle, c):
    if c.kind == "init":
        return oracle.match_initialization(c.F, c.Q, **c.kw)
    return oracle.match_projection(c.F, c.Q, **c.kw)


def _matcher(afv, ctx, c):
    kw = c.kw
    afv.FeatureMatcher.setDescriptorDistanceThresholds(kw.get("th_high", kw.get("th_low")))
    return afv.FeatureMatcher(kw.get("nnratio", 0.8), kw.get("check_orientation", False), ctx=ctx)


def _host(afv, ctx, c):
    """one case through the host-array entry points"""
    m = _matcher(afv, ctx, c)
    try:
        if c.kind == "init":
            return m.SearchForInitialization(c.Q, c.F)
        if c.kw.get("fuse"):
            return m.Fuse(c.F, c.Q)
        return m.SearchByProjection(c.F, c.Q, last_frame=c.kw.get("last_frame", False))
    finally:
        afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_constructed_scene_host_arrays(afv, oracle, gpu_ctx, c):
    want, wn = _oracle(oracle, c)
    got, n = _host(afv, gpu_ctx, c)
    assert n == wn and np.array_equal(got, want)


def _resident(afv, ctx, F):
    """a resident frame holding F's features (afv_frame_set_features): the zero-copy / one-launch ticket path of the searches"""
    fl = F.descriptors.dtype.kind == "f"
    G = dict(min_x=float(F.min_x), min_y=float(F.min_y), grid_cols=F.grid_cols, grid_rows=F.grid_rows)
    # FrameGridView keeps the inverse cell sizes, the frame takes the bounds: the same float32 quotient comes back from these
    G["max_x"] = float(F.min_x) + F.grid_cols / float(F.grid_inv_w)
    G["max_y"] = float(F.min_y) + F.grid_rows / float(F.grid_inv_h)
    fr = afv.Frame(ctx, cap=max(F.N, 1), desc_bytes=32 if fl else F.descriptors.shape[1], float_dim=F.descriptors.shape[1] if fl else 0, **G)
    if fr.grid_inv_w != F.grid_inv_w or fr.grid_inv_h != F.grid_inv_h:
        fr.close()
        return None
    kps = np.zeros(F.N, afv.KP_DTYPE)
    kps["x"], kps["y"] = F.x, F.y
    if F.angles is not None:
        kps["angle"] = F.angles
    fr.set_features(kps, F.descriptors, sizes=F.sizes, u_right=F.u_right)
    return fr


RESIDENT = [c for c in CASES if c.kind == "proj" and not (c.kw.get("fuse") and c.F.inf is not None)]


@pytest.mark.parametrize("c", RESIDENT, ids=[c.name for c in RESIDENT])
def test_constructed_scene_resident_frame(afv, oracle, gpu_ctx, c):
    """(the initialization scenes have their own resident test below; Fuse with the chi-square gate stays with the host arrays: a resident
    frame evaluates the gate on the information values it derived itself, set_features takes none.)"""
    fr = _resident(afv, gpu_ctx, c.F)
    assert fr is not None, "the frame's bounds do not reproduce the scene's cell sizes"
    try:
        m = _matcher(afv, gpu_ctx, c)
        want, wn = _oracle(oracle, c)
        if c.kw.get("fuse"):
            got, n = fr.Fuse(m, c.Q, use_inf_gate=False)
        else:
            got, n = fr.SearchByProjection(m, c.Q, last_frame=c.kw.get("last_frame", False), occupied=c.F.occupied)
        assert n == wn and np.array_equal(got, want)
    finally:
        afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)
        fr.close()


# SearchForInitialization between two resident frames takes vbPrevMatched per query, ONE window size, and the size band 0 .. 1.2^7 with the
# octave-0 filter of F1: a scene is expressible when its queries share one radius.  Left with the host arrays: the skip_* scenes and tie_first
# (two or three radii per scene) and size_lt_min / size_gt_max (per-query bands, which ARE the rule under test).
INIT_HOST_ONLY = ("skip_cx0", "skip_cx1", "skip_cy0", "skip_cy1", "tie_first", "size_lt_min", "size_gt_max")
INIT_RESIDENT = [c for c in CASES if c.kind == "init" and not c.name.startswith(INIT_HOST_ONLY)]


def test_only_the_named_init_scenes_stay_with_the_host_arrays():
    for c in CASES:
        if c.kind == "init":
            one_radius = bool(np.all(c.Q.r == c.Q.r[0]))
            assert one_radius or c.name.startswith(INIT_HOST_ONLY), c.name


@pytest.mark.parametrize("c", INIT_RESIDENT, ids=[c.name for c in INIT_RESIDENT])
def test_constructed_init_scene_between_resident_frames(afv, oracle, gpu_ctx, c):
    """F1 = a resident frame holding the scene's queries as features at (u, v) - octave 0, so all of them search - F2 = the scene's frame;
    the one-launch ranking + ticket hand-off of the initialization on dependency chains, answers behind IK keys, steals, histogram edges"""
    assert c.Q.valid is None and float(c.F.sizes.max()) < 3.0   # inside 0 .. 1.2^7, the band the resident call applies
    f2 = _resident(afv, gpu_ctx, c.F)
    assert f2 is not None, "the frame's bounds do not reproduce the scene's cell sizes"
    fl = c.Q.descriptors.dtype.kind == "f"
    f1 = afv.Frame(gpu_ctx, cap=max(c.Q.n, 1), desc_bytes=32 if fl else c.Q.descriptors.shape[1], float_dim=c.Q.descriptors.shape[1] if fl else 0)
    try:
        kps = np.zeros(c.Q.n, afv.KP_DTYPE)
        kps["x"], kps["y"], kps["angle"] = c.Q.u, c.Q.v, c.Q.angles
        f1.set_features(kps, c.Q.descriptors, sizes=np.ones(c.Q.n, np.float32))
        m = _matcher(afv, gpu_ctx, c)
        want, wn = _oracle(oracle, c)
        # the oracle on what the resident call evaluates (band 0 .. 1.2^7): the same answer, or the scene would not be this scene
        Qb = afv.ProjectionQueries(c.Q.descriptors, c.Q.u, c.Q.v, c.Q.r, np.zeros(c.Q.n, np.float32), np.full(c.Q.n, 3.5831808, np.float32),
                                   angles=c.Q.angles)
        wb, wbn = oracle.match_initialization(c.F, Qb, **c.kw)
        assert wbn == wn and np.array_equal(wb, want)
        got, n = f1.SearchForInitialization(m, f2, np.stack([c.Q.u, c.Q.v], 1), windowSize=float(c.Q.r[0]))
        assert n == wn and np.array_equal(got, want)
    finally:
        afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)
        f1.close(); f2.close()


@pytest.mark.parametrize("name", list(REGIMES))
def test_size_regime_scene(afv, oracle, gpu_ctx, name):
    F, Q = REGIMES[name]
    afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)
    for last, ratio, ori in ((False, 0.8, False), (True, 0.9, True)):
        m = afv.FeatureMatcher(ratio, ori, ctx=gpu_ctx)
        got, n = m.SearchByProjection(F, Q, last_frame=last)
        want, wn = oracle.match_projection(F, Q, th_high=75.0, nnratio=ratio, check_orientation=ori, last_frame=last)
        assert n == wn and np.array_equal(got, want), (last,)
    m = afv.FeatureMatcher(0.9, True, ctx=gpu_ctx)   # (above 32767 queries the fixed point of the initialization steps aside: 16-bit tables)
    got, n = m.SearchForInitialization(Q, F)
    want, wn = oracle.match_initialization(F, Q, th_low=75.0, nnratio=0.9, check_orientation=True)
    assert n == wn and np.array_equal(got, want)
    m = afv.FeatureMatcher(0.6, False, ctx=gpu_ctx)
    got, n = m.Fuse(F, Q)
    want, wn = oracle.match_projection(F, Q, th_high=75.0, fuse=True)
    assert n == wn and np.array_equal(got, want)
    # resident frame: both projection flavours and the gate-less Fuse
    fr = _resident(afv, gpu_ctx, F)
    assert fr is not None, "the frame's bounds do not reproduce the scene's cell sizes"
    try:
        for last, ratio, ori in ((False, 0.8, False), (True, 0.9, True)):
            m = afv.FeatureMatcher(ratio, ori, ctx=gpu_ctx)
            got, n = fr.SearchByProjection(m, Q, last_frame=last, occupied=F.occupied)
            want, wn = oracle.match_projection(F, Q, th_high=75.0, nnratio=ratio, check_orientation=ori, last_frame=last)
            assert n == wn and np.array_equal(got, want), ("resident", last)
        got, n = fr.Fuse(afv.FeatureMatcher(0.6, False, ctx=gpu_ctx), Q, use_inf_gate=False)
        want, wn = oracle.match_projection(F, Q, th_high=75.0, fuse=True)
        assert n == wn and np.array_equal(got, want)
    finally:
        fr.close()


def test_the_library_agrees_with_the_restated_lds_formulas(gpu_ctx):
    import _proj_ref as T
    lib = gpu_ctx.lib
    lib.afv_project_wg_lds.restype = C.c_size_t
    lib.afv_project_wg_lds.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    for n, nq in [(0, 0), (1, 1), (8192, 1), (8192, 1500), (8192, 9000), (8192, 65535), (400, 2500), (63, 65)]:
        assert lib.afv_project_wg_lds(0, n, nq, 0) == T.proj_wg_lds(n, nq)
        assert lib.afv_project_wg_lds(0, n, nq, 1) == T.proj_wg_lds(n, nq, True)
        assert lib.afv_project_wg_lds(1, n, nq, 0) == T.init_wg_lds(n, nq)


def test_size_limits_are_refused_and_the_context_stays_usable(afv, oracle, gpu_ctx):
    """n = 8193, nq = 65536 and 8193 grid cells: AFV_EINVAL before anything is launched; the next valid call answers correctly"""
    ptr = afv._lib.ptr
    m = afv.FeatureMatcher(0.8, False, ctx=gpu_ctx)
    afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)
    good = next(c for c in CASES if c.name == "behind-b32-localmap")
    Fbig, _ = PS.synthetic(8193, 4, 301)
    _, Qbig = PS.synthetic(50, 65536, 302)
    Fcells, Qc = PS.synthetic(100, 10, 303, grid_cols=8193, grid_rows=1)
    Fcells2, _ = PS.synthetic(100, 10, 303, grid_cols=127, grid_rows=65)   # 8255 cells
    for F, Q in ((Fbig, good.Q), (good.F, Qbig), (Fcells, Qc), (Fcells2, Qc)):
        for entry, nout in (("afv_match_projection", F.N), ("afv_match_fuse", Q.n), ("afv_match_initialization", Q.n)):
            j = m._proj_job(F, Q)
            j.th_high = 75.0
            out = np.full(max(nout, 1), -7, np.int32)
            nm = np.full(1, -7, np.int32)
            jobs = (afv._lib.ProjJob * 1)(j)
            assert getattr(gpu_ctx.lib, entry)(gpu_ctx.handle, jobs, 1, ptr(out), ptr(nm)) == EINVAL, entry
            assert np.all(out == -7) and nm[0] == -7   # nothing was written
        got, n = _host(afv, gpu_ctx, good)
        want, wn = _oracle(oracle, good)
        assert n == wn and np.array_equal(got, want)


# ---- job batches ----
def _job(afv, m, F, Q, kw, kind):
    j = m._proj_job(F, Q)
    j.th_high = float(kw.get("th_high", kw.get("th_low", 75.0)))
    j.nnratio = float(kw.get("nnratio", 0.8))
    j.check_orientation = int(bool(kw.get("check_orientation", False)))
    j.mode = afv._lib.PROJ_LASTFRAME if kw.get("last_frame") else afv._lib.PROJ_LOCALMAP
    if kind == "proj" and j.mode == afv._lib.PROJ_LOCALMAP:
        j.check_orientation = 0
    return j


def _run_batch(afv, ctx, entry, items, kind):
    """items: (F, Q, kw).  Returns the per-job (slice, count) of ONE call; outputs follow each other in job order - F.N entries per job for
    the projection searches (feature-indexed), Q.n for Fuse / SearchForInitialization (query-indexed)"""
    m = afv.FeatureMatcher(0.8, False, ctx=ctx)
    jobs = (afv._lib.ProjJob * len(items))(*[_job(afv, m, F, Q, kw, kind) for F, Q, kw in items])
    lens = [F.N if kind == "proj" else Q.n for F, Q, _ in items]
    out = np.full(max(sum(lens), 1), -7, np.int32)
    nm = np.full(len(items), -7, np.int32)
    ctx.check(getattr(ctx.lib, entry)(ctx.handle, jobs, len(items), afv._lib.ptr(out), afv._lib.ptr(nm)), entry)
    res, o = [], 0
    for k, n in enumerate(lens):
        res.append((out[o:o + n].copy(), int(nm[k])))
        o += n
    return res


def _pool(kind):
    """(F, Q, kw) of the constructed scenes a batch draws from, by entry point"""
    if kind == "proj":
        cs = [c for c in CASES if c.kind == "proj" and not c.kw.get("fuse")]
    elif kind == "fuse":
        cs = [c for c in CASES if c.kind == "proj" and c.kw.get("fuse")]
        cs += [c._replace(kw=dict(th_high=75.0, fuse=True)) for c in CASES if c.name.startswith(("behind", "chain")) and c.name.endswith("localmap")]
    else:
        cs = [c for c in CASES if c.kind == "init"]
    return cs


def _special(afv, kind):
    """the jobs every batch carries in its MIDDLE: no queries, no features, every window rejected"""
    F, Q = PS.synthetic(300, 200, 401)
    F0, Q0 = PS.synthetic(0, 40, 402)
    _, Qnone = PS.synthetic(300, 0, 403)
    Fo, Qo = PS.synthetic(300, 150, 404)
    Qo.u = (Qo.u + np.float32(5000.0)).astype(np.float32)
    kw = dict(th_high=75.0, th_low=75.0, nnratio=0.9, last_frame=True, check_orientation=True)
    return [(F, Qnone, kw), (F0, Q0, kw), (Fo, Qo, kw)]


@pytest.mark.parametrize("k", [2, 7, 33])
@pytest.mark.parametrize("kind,entry", [("proj", "afv_match_projection"), ("fuse", "afv_match_fuse"), ("init", "afv_match_initialization")])
def test_job_batches(afv, oracle, gpu_ctx, kind, entry, k):
    """one call with k jobs: different n / nq / grids / widths (32- and 61-byte and float rows together), local-map and last-frame modes,
    occupancy masks and stereo gates on some jobs only.  Every job's slice and count equals the oracle's answer for that job alone AND
    the library's own single-job answer."""
    S = afv.synth
    pool = _pool(kind)
    by_name = {c.name: c for c in CASES}
    item = lambda c: (c.F, c.Q, c.kw)
    first = lambda tag, start="": item(next(c for c in pool if tag in c.name + "-" and c.name.startswith(start)))
    ikw = dict(th_high=75.0, th_low=75.0, nnratio=0.9, check_orientation=True)
    # a job with the stereo fields set (an undistorted grid as well) and one with an occupancy mask and non-occupying queries
    stereo = by_name["uright_ge0-b32-fuse-undist" if kind == "fuse" else "er_gt_max-b32-localmap-undist"]
    stereo = (stereo.F, stereo.Q, ikw if kind == "init" else stereo.kw)
    assert stereo[0].u_right is not None and stereo[1].ur is not None
    F, Q = REGIMES["live2500-rescans"]   # much larger than the rest (wg_lds / stage_cap are sized by it), occupancy mask, qoccupies
    big = (F, Q, dict(th_high=75.0, th_low=75.0, nnratio=0.8, check_orientation=True))
    assert F.occupied is not None and F.occupied.any() and Q.occupies is not None and not Q.occupies.all()
    if k == 2:
        items = [first("-f8-", "behind"), first("-b32-", "behind")]   # a float job ahead of a binary one
    elif k == 7:   # every slot by hand: the three special jobs in the middle
        items = [first("-b61-"), big] + _special(afv, kind) + [first("-f8-"), stereo]
    else:
        pick = (S.lcg_states(900 + k, k) % len(pool)).tolist()
        items = [item(pool[i]) for i in pick]
        items[0], items[1], items[2], items[3], items[4], items[32] = first("-b61-"), big, first("-coarse"), first("-f64-"), stereo, first("-f8-")
        items[5] = first("-b32-", "behind")   # features occupied before the call
        items[15:18] = _special(afv, kind)
        F, Q = REGIMES["n8192-nq1500"]       # too large for the fixed point: the whole call takes the ordered walk
        items[20] = (F, Q, dict(th_high=75.0, th_low=75.0, nnratio=0.8))
        F, Q = REGIMES["grid-8192-cells"]
        items[21] = (F, Q, dict(th_high=75.0, th_low=75.0, nnratio=0.9, last_frame=True, check_orientation=True))
    assert len(items) == k
    if k >= 7:
        assert sum(1 for F, Q, _ in items if Q.n == 0) == 1 and sum(1 for F, Q, _ in items if F.N == 0) == 1
        assert any(Q.n and float(Q.u.min()) > 4000 for F, Q, _ in items)   # every window rejected
        assert 0 < sum(1 for F, Q, _ in items if F.occupied is not None) < k and 0 < sum(1 for F, Q, _ in items if F.u_right is not None) < k
    got = _run_batch(afv, gpu_ctx, entry, items, kind)
    for i, (F, Q, kw) in enumerate(items):
        if kind == "init":
            want, wn = oracle.match_initialization(F, Q, th_low=kw.get("th_low", kw.get("th_high", 75.0)), nnratio=kw.get("nnratio", 0.8),
                                                   check_orientation=kw.get("check_orientation", False))
        elif kind == "fuse":
            want, wn = oracle.match_projection(F, Q, th_high=kw.get("th_high", 75.0), fuse=True)
        else:
            last = bool(kw.get("last_frame"))
            want, wn = oracle.match_projection(F, Q, th_high=kw.get("th_high", 75.0), nnratio=kw.get("nnratio", 0.8),
                                               check_orientation=last and kw.get("check_orientation", False), last_frame=last)
        assert got[i][1] == wn and np.array_equal(got[i][0], want), ("job %d of %d differs from the oracle" % (i, k))
        single = _run_batch(afv, gpu_ctx, entry, [items[i]], kind)[0]
        assert single[1] == got[i][1] and np.array_equal(single[0], got[i][0]), ("job %d of %d differs from the single-job call" % (i, k))


# ---- one scene through every route ----
def _points_scene(flavour, desc):
    """65 ids of a seeded map-point scene against its first 70 features, a few of them occupied before a FRUSTUM search; desc "f64": the
    same geometry with rows of 64 floats"""
    import _points_scenes as MS
    import test_gpu_points as TP
    base = TP.random_scene(1, flavour)
    P, feat = TP._with_rows(base, 256, 64) if desc == "f64" else (base.P, base.feat)
    feat = MS.Features(feat.x[:70], feat.y[:70], feat.sizes[:70], feat.desc[:70], angles=feat.angles[:70])
    occ = None
    if flavour == TP.R.FRUSTUM:
        occ = np.zeros(70, np.uint8)
        occ[[2, 9, 30]] = 1
    return MS.Scene(base.name + "-65", None, flavour, P, base.cam, base.ids[:65], None, radius_th=base.radius_th, feat=feat, th=64.0,
                    nnratio=base.nnratio, occupied=occ)


@pytest.mark.parametrize("desc", ["b32", "f64"])
def test_one_scene_through_every_projection_route(afv, oracle, gpu_ctx, desc):
    """PS.every_route_scene through every entry point that can state it - host arrays alone and as the middle job of a batch of three, a
    resident frame with the queries' rows by value and by reference into a keyframe table, with and without the occupancy mask and the
    stereo gate, Fuse alone / as one direction of a SearchBySim3 pair / against the frame with and without the chi-square gate,
    SearchForInitialization from host arrays and between two resident frames - and a map-point scene of the same size through ids: every
    answer equals the oracle's AND the host-array answer, so a pointer taken from the wrong base on one route shows as a difference.
    tests/test_proj_ref_cpu.py shows that the scene's answer hangs on its masks and its histogram."""
    import copy
    import test_gpu_points as TP
    s = PS.every_route_scene(desc)
    F, Q, Fs, Qs, Qi, F1, Q2 = (s[k] for k in ("F", "Q", "Fs", "Qs", "Qi", "F1", "Q2"))
    assert F.N == 70 and Q.n == 65 and (F.grid_cols, F.grid_rows) == (64, 48)
    fl = desc == "f64"
    afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)
    same = lambda got, want, what: (got[1] == want[1] and np.array_equal(got[0], want[0])) or pytest.fail(what)
    fr = _resident(afv, gpu_ctx, Fs)   # carries mvuRight: the plane takes part only when the queries bring their side of the gate
    assert fr is not None
    f1 = afv.Frame(gpu_ctx, cap=Q.n, desc_bytes=32, float_dim=64 if fl else 0)
    table = afv.table.DescriptorTable(gpu_ctx, 2, 40, float_dim=64) if fl else afv.table.DescriptorTable(gpu_ctx, 2, 40, desc_bytes=32)
    rigs = []
    try:
        # SearchByProjection(CurrentFrame, LastFrame) with the orientation check
        kw = dict(th_high=75.0, nnratio=0.9, check_orientation=True, last_frame=True)
        m = afv.FeatureMatcher(0.9, True, ctx=gpu_ctx)
        slots = (np.arange(Q.n) % 2).astype(np.int32)
        idx = (np.arange(Q.n) // 2).astype(np.int32)
        for sl in (0, 1):
            table.set(sl, Q.descriptors[slots == sl])
        Fa, Qa = PS.synthetic(33, 17, 978)
        Fb, Qb = PS.synthetic(21, 40, 979)
        for masked in (True, False):
            Fm = F if masked else copy.copy(F)
            if not masked:
                Fm.occupied = None
            want = oracle.match_projection(Fm, Q, **kw)
            host = m.SearchByProjection(Fm, Q, last_frame=True)
            same(host, want, ("host arrays", masked))
            batch = _run_batch(afv, gpu_ctx, "afv_match_projection", [(Fa, Qa, kw), (Fm, Q, kw), (Fb, Qb, kw)], "proj")
            same(batch[1], host, ("middle of a batch of three", masked))
            same(batch[0], oracle.match_projection(Fa, Qa, **kw), "first of the batch")
            same(batch[2], oracle.match_projection(Fb, Qb, **kw), "last of the batch")
            same(fr.SearchByProjection(m, Q, last_frame=True, occupied=Fm.occupied), host, ("resident frame, rows by value", masked))
            same(fr.SearchByProjection(m, Q, last_frame=True, occupied=Fm.occupied, qref=(table, slots, idx)), host,
                 ("resident frame, rows by reference", masked))
        want = oracle.match_projection(Fs, Qs, **kw)
        assert not np.array_equal(want[0], oracle.match_projection(F, Q, **kw)[0])   # the gate decides something
        host = m.SearchByProjection(Fs, Qs, last_frame=True)
        same(host, want, "host arrays, stereo")
        same(fr.SearchByProjection(m, Qs, last_frame=True, occupied=Fs.occupied), host, "resident frame, stereo")
        # Fuse
        m6 = afv.FeatureMatcher(0.6, False, ctx=gpu_ctx)
        fkw = dict(th_high=75.0, fuse=True)
        want = oracle.match_projection(F, Q, **fkw)
        back = oracle.match_projection(F1, Q2, **fkw)
        host = m6.Fuse(F, Q)
        same(host, want, "Fuse, host arrays")
        pair = _run_batch(afv, gpu_ctx, "afv_match_fuse", [(F, Q, fkw), (F1, Q2, fkw)], "fuse")
        same(pair[0], host, "Fuse, first of two jobs")
        same(pair[1], back, "Fuse, second of two jobs")
        m12 = pair[0][0].copy()
        hit = m12 >= 0
        m12[hit] = np.where(pair[1][0][m12[hit]] == np.flatnonzero(hit), m12[hit], -1)
        sim3 = m.SearchBySim3(F1, Q, F, Q2)
        same(sim3, (m12, int((m12 >= 0).sum())), "SearchBySim3 = the two directions where they agree")
        same(sim3, oracle.match_sim3(F, Q, F1, Q2, th_high=75.0), "SearchBySim3")
        same(fr.Fuse(m6, Q, use_inf_gate=False), host, "Fuse, resident frame, no gate")
        Fi = copy.copy(F)
        Fi.inf = (np.float32(1.0) / (F.sizes * F.sizes)).astype(np.float32)   # keyPtsInf as a frame derives it from keyPtsSize
        want = oracle.match_projection(Fi, Q, **fkw)
        assert want[1] < host[1]                                              # the gate rejects something
        gated = m6.Fuse(Fi, Q)
        same(gated, want, "Fuse with the chi-square gate, host arrays")
        same(fr.Fuse(m6, Q, use_inf_gate=True), gated, "Fuse with the chi-square gate, resident frame")
        # SearchForInitialization
        ikw = dict(th_low=75.0, nnratio=0.9, check_orientation=True)
        same(m.SearchForInitialization(Q, F), oracle.match_initialization(F, Q, **ikw), "initialization, host arrays, masked queries")
        want = oracle.match_initialization(F, Qi, **ikw)
        host = m.SearchForInitialization(Qi, F)
        same(host, want, "initialization, host arrays")
        kps = np.zeros(Q.n, afv.KP_DTYPE)
        kps["x"], kps["y"], kps["angle"] = Q.u, Q.v, Q.angles
        f1.set_features(kps, Q.descriptors, sizes=np.ones(Q.n, np.float32))
        same(f1.SearchForInitialization(m, fr, np.stack([Q.u, Q.v], 1), windowSize=float(Q.r[0])), host, "initialization, resident frames")
        # map points by id: check_search holds the search through ids to the restatement and to afv_frame_match_projection / _fuse fed with
        # the projected queries
        for flavour in (TP.R.FRUSTUM, TP.R.FUSE):
            sc = _points_scene(flavour, desc)
            rigs.append(TP.Rig(afv, gpu_ctx, sc, P=sc.P, feat=sc.feat))
            assert TP.check_search(afv, rigs[-1], sc) >= 5
    finally:
        afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)
        for r in rigs:
            r.close()
        table.close(); f1.close(); fr.close()
