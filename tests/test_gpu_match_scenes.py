"""-m gpu: the constructed scenes of tests/_match_scenes.py through every route that reaches k_match_bow, k_match_bow_seg (both bodies),
k_match_bow_finish, the top-4 + resolve path and k_match_tri.  Bar: every output index and the count equal to the oracle's
(tests/test_match_ref_cpu.py proves on the CPU that the oracle equals the restated reference on these scenes and that each scene reaches
its rule).  A test walks many scenes and reports the names of ALL that differ.
"""
import ctypes

import numpy as np
import pytest

import _match_scenes as MS

pytestmark = pytest.mark.gpu

CASES = MS.all_constructed()
BATCHES = MS.batches(CASES)
_WANT = {}


def want_of(oracle, c):
    if c.name not in _WANT:
        _WANT[c.name] = MS.run_oracle(oracle, c)
    return _WANT[c.name]


@pytest.fixture(scope="module")
def matcher(afv, gpu_ctx):
    return afv.FeatureMatcher(0.6, True, ctx=gpu_ctx)


@pytest.fixture(autouse=True)
def settings_restored(afv, matcher):
    """run_host sets the class-wide thresholds and the matcher's ratio / orientation switch per scene: every test leaves them as it found
    them, so that nothing here or in another file depends on the order of the tests"""
    FM = afv.FeatureMatcher
    names = ("TH_LOW", "TH_HIGH", "descDistTh_low_reloc", "descDistTh_high_reloc")
    before = [getattr(FM, n) for n in names] + [matcher.mfNNratio, matcher.mbCheckOrientation]
    yield
    for n, v in zip(names, before):
        setattr(FM, n, v)
    matcher.mfNNratio, matcher.mbCheckOrientation = before[4], before[5]


def bow_jobs(afv, matcher, cases):
    """one afv_match_bow call over jobs that may differ in mode, descriptor kind, thresholds and orientation check.  The raw call stands in
    for FeatureMatcher.SearchByBoW_batch here because that wrapper gives every job of a call one mode and the matcher's one set of
    settings; test_uniform_batches_through_the_python_wrapper runs what it can express"""
    lib = afv._lib
    keep, jobs, nouts = [], [], []
    for c in cases:
        j = matcher._job(c.K1, c.K2, lib.MATCH_KF_FRAME if c.kind == "kff" else lib.MATCH_KF_KF, keep)
        j.th_low, j.nnratio, j.check_orientation = c.kw["th_low"], c.kw["nnratio"], int(c.kw["check_orientation"])
        jobs.append(j); nouts.append(c.K2.N if c.kind == "kff" else c.K1.N)
    arr = (lib.MatchJob * len(jobs))(*jobs)
    out = np.full(max(sum(nouts), 1), -7, np.int32)
    nm = np.full(len(jobs), -7, np.int32)
    matcher.ctx.check(matcher.lib.afv_match_bow(matcher.ctx.handle, arr, len(jobs), lib.ptr(out), lib.ptr(nm)), "afv_match_bow")
    res, o = [], 0
    for k, n in enumerate(nouts):
        res.append((out[o:o + n].copy(), int(nm[k]))); o += n
    return res


def tri_jobs(afv, matcher, cases):
    lib = afv._lib
    keep, jobs = [], []
    for c in cases:
        t = lib.sized(lib.TriJob)
        t.bow = matcher._job(c.K1, c.K2, lib.MATCH_KF_KF, keep)
        t.bow.th_low = c.kw["th_low"]
        arrs = [np.ascontiguousarray(a, np.float32) for a in (c.K1.pts[:, 0], c.K1.pts[:, 1], c.K2.pts[:, 0], c.K2.pts[:, 1], c.K2.sigma2)]
        keep += arrs
        t.x1, t.y1, t.x2, t.y2, t.sigma2_2 = [lib.ptr(a) for a in arrs]
        for i, v in enumerate(np.asarray(c.kw["F12"], np.float32).reshape(9)):
            t.F12[i] = float(v)
        t.ex, t.ey = float(c.kw["epipole"][0]), float(c.kw["epipole"][1])
        t.u_right1, t.u_right2 = lib.ptr(c.K1.u_right), lib.ptr(c.K2.u_right)
        t.only_stereo = int(bool(c.kw.get("only_stereo", False)))
        jobs.append(t)
    arr = (lib.TriJob * len(jobs))(*jobs)
    out = np.full(max(sum(c.K1.N for c in cases), 1), -7, np.int32)
    nm = np.full(len(jobs), -7, np.int32)
    matcher.ctx.check(matcher.lib.afv_match_triangulation(matcher.ctx.handle, arr, len(jobs), lib.ptr(out), lib.ptr(nm)), "afv_match_triangulation")
    res, o = [], 0
    for k, c in enumerate(cases):
        res.append((out[o:o + c.K1.N].copy(), int(nm[k]))); o += c.K1.N
    return res


def run_host(afv, matcher, c):
    """the public methods of FeatureMatcher, one scene"""
    afv.FeatureMatcher.setDescriptorDistanceThresholds(float(c.kw["th_low"]))
    if c.kind == "tri":
        pairs, n = matcher.SearchForTriangulation(c.K1, c.K2, c.kw["F12"], c.kw["epipole"], c.kw.get("only_stereo", False))
        got = np.full(c.K1.N, -1, np.int32)
        for a, b in pairs:
            got[a] = b
        return got, n
    matcher.mfNNratio, matcher.mbCheckOrientation = float(c.kw["nnratio"]), bool(c.kw["check_orientation"])
    return matcher.SearchByBoW(c.K1, c.K2, frame=(c.kind == "kff"))


def differing(oracle, cases, results):
    bad = []
    for c, (got, n) in zip(cases, results):
        want, wn = want_of(oracle, c)
        if n != wn or not np.array_equal(got, want):
            bad.append(c.name)
    return bad


def _eligible(c):
    """afv_match_bow_impl takes the top-4 + resolve path when EVERY job of a call looks like this"""
    return (c.kind == "kfkf" and c.K1.featvec is None and c.K1.descriptors.dtype == np.uint8 and c.K1.descriptors.shape[1] == 32 and
            c.K1.valid is None and c.K2.valid is None and max(c.K1.N, c.K2.N) <= 4096)


def test_every_scene_through_the_host_array_methods(afv, oracle, matcher):
    """FeatureMatcher.SearchByBoW(frame=False / True) and SearchForTriangulation, one scene per call"""
    res = [run_host(afv, matcher, c) for c in CASES]
    assert differing(oracle, CASES, res) == []


@pytest.mark.parametrize("path", ["batch-kernels", "small-batch-kernels", "batch-kernels, one-wavefront walk"])
@pytest.mark.parametrize("engine", [0, 1])
def test_fast_path_scenes_under_every_engine_and_resolve(afv, oracle, matcher, gpu_ctx, engine, path):
    """the scenes and batches that afv_match_bow sends to the top-4 + resolve path, under the three settings of tests/test_gpu_match.py's
    pairs_path and both phase-1 engines; the library's own choices are restored afterwards"""
    cases = [c for c in CASES if _eligible(c)]
    assert len(cases) >= 12 and any(c.name.startswith("chain-") for c in cases) and any(c.name.startswith("behind-") for c in cases)
    gpu_ctx.set_small_batch_path(2 if path == "small-batch-kernels" else 0)
    gpu_ctx.set_match_resolve(0 if "walk" in path else 1)
    gpu_ctx.set_match_engine(engine)
    try:
        bad = differing(oracle, cases, [run_host(afv, matcher, c) for c in cases])
        for name in ("fast-path-settings", "fast-path-but-one"):
            bad += ["%s/%s" % (name, b) for b in differing(oracle, BATCHES[name], bow_jobs(afv, matcher, BATCHES[name]))]
        bad += ["all-eligible/" + b for b in differing(oracle, cases, bow_jobs(afv, matcher, cases))]
    finally:
        gpu_ctx.set_match_engine(1)
        gpu_ctx.set_small_batch_path(1)
        gpu_ctx.set_match_resolve(2)
    assert bad == []


@pytest.mark.parametrize("name", list(BATCHES))
def test_mixed_batches_give_every_job_its_solo_answer(afv, oracle, matcher, name):
    """the kernel form is chosen per CALL (per_node when any job has more than one shared node; the top-4 path when every job is eligible):
    a job's answer must not depend on its neighbours.  (KF, KF) and (KF, F) jobs, 20 / 32 / 61-byte and float rows, zero, one and many
    shared nodes, different th_low / nnratio / check_orientation in one afv_match_bow / afv_match_triangulation call"""
    cases = BATCHES[name]
    res = tri_jobs(afv, matcher, cases) if name.startswith("tri-") else bow_jobs(afv, matcher, cases)
    assert differing(oracle, cases, res) == []
    again = tri_jobs(afv, matcher, cases[::-1]) if name.startswith("tri-") else bow_jobs(afv, matcher, cases[::-1])
    assert differing(oracle, cases[::-1], again) == []


def test_uniform_batches_through_the_python_wrapper(afv, oracle, matcher):
    """FeatureMatcher.SearchByBoW_batch: the jobs of the mixed batches regrouped into calls of one mode and one set of settings each
    (what the wrapper can say), every group with 2 jobs or more in one call"""
    groups = {}
    for name, cases in BATCHES.items():
        if name.startswith("tri-"):
            continue
        for c in cases:
            groups.setdefault((c.kind, c.kw["th_low"], c.kw["nnratio"], bool(c.kw["check_orientation"])), {})[c.name] = c
    ran, bad = 0, []
    for (kind, th, ratio, ori), members in groups.items():
        cases = list(members.values())
        if len(cases) < 2:
            continue
        afv.FeatureMatcher.setDescriptorDistanceThresholds(float(th))
        matcher.mfNNratio, matcher.mbCheckOrientation = float(ratio), ori
        bad += differing(oracle, cases, matcher.SearchByBoW_batch([(c.K1, c.K2) for c in cases], frame=(kind == "kff")))
        ran += len(cases)
    assert bad == [] and ran >= 30 and len(groups) >= 6


def _one_node(afv, K):
    """a side without a FeatureVector, as a table slot holds it: one node listing every feature (the same segment as brute force)"""
    if K.featvec is not None:
        return K
    return afv.FeatureView(K.descriptors, [(1, list(range(K.N)))], K.valid, K.angles, K.pts, K.sigma2, K.u_right)


@pytest.mark.parametrize("desc", ["b32", "b61", "f64"])
def test_rule_scenes_through_keyframe_table_slots(afv, oracle, gpu_ctx, desc):
    """DescriptorTable.match_bow, match_bow_frame (host frame view) and match_triangulation over slots 0 / 1: the three table kinds that
    exist.  The other descriptor kinds stay on host arrays"""
    cases = [c for c in CASES if c.rule is not None and ("-%s-" % desc) in c.name]
    assert len(cases) > 100
    cap = max(max(c.K1.N, c.K2.N) for c in cases)
    kw = dict(float_dim=64) if desc == "f64" else dict(desc_bytes=int(desc[1:]))
    table = afv.table.DescriptorTable(gpu_ctx, 2, cap, **kw)
    bad = []
    for c in cases:
        K1, K2 = _one_node(afv, c.K1), _one_node(afv, c.K2)
        want, wn = want_of(oracle, c)
        for slot, K in ((0, K1), (1, K2)):
            if c.kind == "kff" and slot == 1:
                continue
            table.set(slot, K.descriptors, K.angles)
            table.set_featvec(slot, *K.csr()[:3])
            table.set_valid(slot, None if c.kind == "tri" else K.valid)
            if c.kind == "tri":
                table.set_geometry(slot, K.pts[:, 0], K.pts[:, 1], K.sigma2 if K.sigma2 is not None else np.ones(K.N, np.float32), K.u_right)
        if c.kind == "kfkf":
            m, nm = table.match_bow([0], [1], c.kw["th_low"], c.kw["nnratio"], c.kw["check_orientation"])
            got = m[0, :K1.N]
        elif c.kind == "kff":
            m, nm = table.match_bow_frame([0], K2, c.kw["th_low"], c.kw["nnratio"], c.kw["check_orientation"])
            got = m[0]
        else:
            m, nm = table.match_triangulation([0], [1], np.asarray(c.kw["F12"], np.float32)[None], np.asarray(c.kw["epipole"], np.float32)[None],
                                              c.kw["th_low"], [K1.valid], [K2.valid], c.kw.get("only_stereo", False))
            got = m[0, :K1.N]
        if int(nm[0]) != wn or not np.array_equal(got, want):
            bad.append(c.name)
    table.close()
    assert bad == []


@pytest.mark.parametrize("desc", ["b32", "b61", "f64"])
def test_resident_frame_as_the_frame_side(afv, oracle, gpu_ctx, desc):
    """DescriptorTable.match_bow_frame_resident, the three table kinds.  A resident frame's FeatureVector is whatever Frame::ComputeBoW makes
    of its descriptors: ascending indices, the vocabulary's nodes.  The hand-built FeatureVectors of the rule scenes (listed orders,
    chosen node ids, filler placed first) cannot be installed in a resident frame through the existing API, so that part of the scenes
    stays with the table's host-frame route above.  What can be produced is used: the DESCRIPTORS of every (KF, F) rule scene in all
    three shapes (they differ in their filler rows here), set_features into a frame, ComputeBoW on the device, the keyframe's
    FeatureVector from the same vocabulary on the host; the oracle gets the same two vectors"""
    if desc == "f64":
        voc = afv.Vocabulary.random_float(3, k=8, L=3, ctx=gpu_ctx, dim=64)
        fr = afv.Frame(gpu_ctx, float_dim=64)
        kw = dict(float_dim=64)
    else:
        voc = afv.Vocabulary.random(3, k=8, L=3, ctx=gpu_ctx, desc_bytes=int(desc[1:]))
        fr = afv.Frame(gpu_ctx, desc_bytes=int(desc[1:]))
        kw = dict(desc_bytes=int(desc[1:]))
    cases = [c for c in CASES if c.rule is not None and c.kind == "kff" and ("-%s-" % desc) in c.name]
    assert len(cases) > 45
    cap = max(max(c.K1.N, c.K2.N) for c in cases)
    table = afv.table.DescriptorTable(gpu_ctx, 1, cap, **kw)
    bad, matched = [], 0
    for c in cases:
        kps = np.zeros(c.K2.N, afv.KP_DTYPE)
        kps["x"] = 20.0 + 2.0 * np.arange(c.K2.N); kps["y"] = 30.0; kps["size"] = 31.0; kps["angle"] = c.K2.angles
        fr.set_features(kps, c.K2.descriptors)
        _, fv2 = fr.ComputeBoW(voc, levelsup=2)
        assert fr.featvec() == fv2
        _, fv1 = voc.transform(c.K1.descriptors, levelsup=2)
        table.set(0, c.K1.descriptors, c.K1.angles)
        table.set_featvec(0, *afv.FeatureView(c.K1.descriptors, fv1).csr()[:3])
        table.set_valid(0, c.K1.valid)
        m, nm = table.match_bow_frame_resident([0], fr, c.kw["th_low"], c.kw["nnratio"], c.kw["check_orientation"])
        want, wn = oracle.search_by_bow_kf_frame(c.K1.descriptors, c.K2.descriptors, fv1, fv2, c.K1.valid, c.K1.angles, c.K2.angles,
                                                 c.kw["th_low"], c.kw["nnratio"], c.kw["check_orientation"])
        matched += wn
        if int(nm[0]) != wn or not np.array_equal(m[0], want):
            bad.append(c.name)
    fr.close(); table.close(); voc.close()
    assert bad == [] and matched > 100


def test_a_side_of_8193_is_refused(afv, matcher):
    """AFV_MAX_SIDE = 8192: refused with AfvError by validate_job, before anything is staged or launched"""
    afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)
    for K1, K2 in MS.too_large():
        for frame in (False, True):
            with pytest.raises(afv._lib.AfvError):
                matcher.SearchByBoW(K1, K2, frame=frame)
        K1.pts = np.zeros((K1.N, 2), np.float32); K2.pts = np.zeros((K2.N, 2), np.float32); K2.sigma2 = np.ones(K2.N, np.float32)
        with pytest.raises(afv._lib.AfvError):
            matcher.SearchForTriangulation(K1, K2, MS.F_HLINE, MS.FAR_EPIPOLE)


def _twice(afv, n, fv):
    """a FeatureView whose FeatureVector lists a feature twice, past the Python layer's own check (FeatureView.csr refuses it, see
    tests/test_match_ref_cpu.py): the C entry points must refuse it themselves"""
    K = afv.FeatureView(afv.synth.random_descriptors(3, n), None, None, np.zeros(n, np.float32), np.zeros((n, 2), np.float32), np.ones(n, np.float32))
    ids = np.array([i for i, _ in fv], np.int32)
    ptrs = np.cumsum([0] + [len(l) for _, l in fv]).astype(np.int32)
    flat = np.array([i for _, l in fv for i in l], np.int32)
    K.featvec = fv
    K._csr = (ids, ptrs, flat, len(fv))
    return K


def test_a_feature_listed_twice_is_refused_by_every_entry_point(afv, matcher, gpu_ctx):
    """total <= n alone lets ([0, 1], [1, 2]) of 4 features pass; the per-node kernels index their taken flags by position in the node and
    two nodes would write one output slot.  AFV_EINVAL before anything is staged; nothing of this input ever reaches a kernel"""
    E = afv._lib.AfvError
    afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)
    good = [(1, [0, 1]), (5, [2, 3])]
    for bad_fv in ([(1, [0, 1]), (5, [1, 2])], [(1, [3, 3])], [(1, [0]), (2, []), (9, [2, 3, 0])]):
        with pytest.raises(E):
            afv.FeatureView(afv.synth.random_descriptors(3, 4), bad_fv).csr()
        for A, B in ((_twice(afv, 4, bad_fv), _twice(afv, 4, good)), (_twice(afv, 4, good), _twice(afv, 4, bad_fv))):
            for frame in (False, True):
                with pytest.raises(E) as e:
                    matcher.SearchByBoW(A, B, frame=frame)
                assert e.value.code == afv._lib.EINVAL
            with pytest.raises(E) as e:
                matcher.SearchForTriangulation(A, B, MS.F_HLINE, MS.FAR_EPIPOLE)
            assert e.value.code == afv._lib.EINVAL
        table = afv.table.DescriptorTable(gpu_ctx, 2, 8)
        K = _twice(afv, 4, bad_fv)
        table.set(0, K.descriptors, K.angles)
        with pytest.raises(E) as e:
            table.set_featvec(0, *K.csr()[:3])
        assert e.value.code == afv._lib.EINVAL
        table.set_featvec(0, *_twice(afv, 4, good).csr()[:3])     # the slot still takes a proper one
        with pytest.raises(E) as e:
            table.match_bow_frame([0], K, 75.0, 0.7, True)
        assert e.value.code == afv._lib.EINVAL
        m, nm = table.match_bow_frame([0], _twice(afv, 4, good), 75.0, 0.7, True)
        assert nm[0] == 4 and m[0].tolist() == [0, 1, 2, 3]
        table.close()


def test_one_scene_through_every_bow_route(afv, oracle, matcher, gpu_ctx):
    """MS.every_route_scene (70 x 65 features of 32 bytes, 3 shared nodes and 1 unshared on each side, masks, check_orientation on) through
    the five routes that end in the BoW-guided kernels: the host-array (KF, KF) job alone; the same job behind a single-segment job with
    n2 = 0 in one call; table slots of cap 80; the table against a host frame view; the table against a resident frame whose
    FeatureVector the device computed.  The three (KF, KF) answers equal the oracle's search_by_bow_kf_kf and the two (KF, F) answers
    its search_by_bow_kf_frame - the two rules differ (th_low strict or not, the frame-side mask, the key of the rotation histogram), so
    a route is compared with the routes of its own rule - bit for bit on the n entries a layout holds for the job; the padded tail of
    the table layout is -1; a frame without features leaves match_f alone and counts 0 for every slot"""
    lib = afv._lib
    kfkf, kff, voc_args = MS.every_route_scene()
    K1, K2 = kfkf.K1, kfkf.K2
    kw = kfkf.kw
    (want12, n12), (want_f, n_f) = MS.run_oracle(oracle, kfkf), MS.run_oracle(oracle, kff)
    assert n12 > 30 and n_f > 30 and n12 != n_f
    got = {}
    got["host"] = bow_jobs(afv, matcher, [kfkf])[0]
    none = afv.FeatureView(afv.synth.random_descriptors(5, 7), None, None, np.zeros(7, np.float32))
    nothing = afv.FeatureView(np.zeros((0, 32), np.uint8), None, None, np.zeros(0, np.float32))
    other = MS.Case("single-segment-n2-0", "kfkf", none, nothing, dict(kw, check_orientation=False), None)
    (m_other, n_other), got["batch"] = bow_jobs(afv, matcher, [other, kfkf])
    assert n_other == 0 and m_other.tolist() == [-1] * 7
    table = afv.table.DescriptorTable(gpu_ctx, 2, 80)
    for slot, K in ((0, K1), (1, K2)):
        table.set(slot, K.descriptors, K.angles)
        table.set_featvec(slot, *K.csr()[:3])
        table.set_valid(slot, K.valid)
    m, nm = table.match_bow([0], [1], kw["th_low"], kw["nnratio"], True)
    assert m.shape == (1, 80) and np.all(m[0, K1.N:] == -1)
    got["slots"] = (m[0, :K1.N], int(nm[0]))
    m, nm = table.match_bow_frame([0], K2, kw["th_low"], kw["nnratio"], True)
    got["view"] = (m[0], int(nm[0]))
    voc = afv.Vocabulary(*voc_args, ctx=gpu_ctx)
    fr = afv.Frame(gpu_ctx)
    kps = np.zeros(K2.N, afv.KP_DTYPE)
    kps["x"], kps["y"], kps["size"], kps["angle"] = K2.pts[:, 0], K2.pts[:, 1], 31.0, K2.angles
    fr.set_features(kps, K2.descriptors)
    fr.ComputeBoW(voc, levelsup=1)
    assert fr.featvec() == K2.featvec
    m, nm = table.match_bow_frame_resident([0], fr, kw["th_low"], kw["nnratio"], True)
    got["resident"] = (m[0], int(nm[0]))
    # a frame without features: counts 0 for both slots, match_f untouched
    view = lib.FrameView(None, 0, None, None, None, None, 0)
    slots = np.array([0, 1], np.int32)
    match_f = np.full(8, -7, np.int32)
    counts = np.full(2, -7, np.int32)
    gpu_ctx.check(table.lib.afv_table_match_bow_frame(table.handle, lib.ptr(slots), 2, ctypes.byref(view), kw["th_low"], kw["nnratio"], 1,
                                                      lib.ptr(match_f), lib.ptr(counts)), "afv_table_match_bow_frame")
    fr.close(); voc.close(); table.close()
    assert counts.tolist() == [0, 0] and np.all(match_f == -7)
    bad = [r for r in ("host", "batch", "slots") if got[r][1] != n12 or not np.array_equal(got[r][0], want12)]
    bad += [r for r in ("view", "resident") if got[r][1] != n_f or not np.array_equal(got[r][0], want_f)]
    assert bad == []
