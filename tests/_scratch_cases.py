"""The cases of tests/test_gpu_scratch.py: one row per device entry point that stages through a context, and the list of the entry points
left out (tests/test_scratch_cases_cpu.py holds the two lists to include/afv_hip.h).

A row names its C entry points and gives make(afv, ctx, oracle) -> step.  step() builds the module's own rig on `ctx`, makes the call
and holds the answer to the expected one with the module's own equality (bits; a NaN equals a NaN where that module says so) - the rigs,
scenes, cached restatement answers and oracle calls of the existing test modules, nothing new.  Most steps ARE a test function of such a
module, called with the fresh context in the place of the session's (`reuse`): its rig is then built, used and closed inside every step,
so the stores and tables of such a row are new allocations in every pass and only the context's own buffers are painted under it.  The
rows marked `holds` keep their store or table alive across the three passes (made in make(), closed by step.close): there the setters
of the store (afv_points_set / _set_flags / _set_descriptors), afv_points_get and afv_table_match_pairs run on painted d_stage / h_pin
and d_pairs / d_out / d_nm / h_pin, and the test asserts that those buffers were there to be painted.  The test wraps the library's
symbols while a step runs and asserts that every entry point the row names was really called.

WHAT THE HOST CODE LAYS INTO d_match / h_stage, read from csrc/ before the first painted run.  `in` = an uploaded input (Blob::put), `zero`
= Blob::reserve (zero in the image and uploaded with the inputs unless noted), `scratch` = Blob::reserve_scratch / take: neither filled
nor copied, so it must be written by a kernel (or a fill) of the same call before anything reads it.  Every region that holds indices,
offsets or counts a kernel uses as an address is `in` or `zero` unless the line says which kernel writes it first.
  afv_poseopt.hip     in: pts, poses.  scratch: out records, outlier flags - written by k_pose_optimize, fetched.
  afv_pnp.hip         in: candidates, pts rows.  scratch: n, min_inliers, index, p2d, p3dw, max_err (k_pnp_gather writes them, the first of
                      the three launches), count / degenerate / pose / inliers (k_pnp_hypotheses), refined* (k_pnp_refine); all fetched.
  afv_init.hip        in: matches12.  scratch: n, pairs, norm (k_init_prepare, first launch), sets / score / model / degenerate / inliers
                      (k_init_hypotheses), cos / p3dk / status / trace / answer / Rt / p3d / triangulated (k_init_reconstruct).
  afv_sim3.hip        in: jobs, slots, mp1, mp2, idx1, idx2.  scratch: n, index1, x3dc, image points, max_err (k_sim3_gather, first launch),
                      count / degenerate / sim3 / inliers (k_sim3_hypotheses).
  afv_sim3opt.hip     in: jobs, mp1, mp2, idx2.  scratch: n, index1, edges, active, results, state (k_sim3opt_gather, then _solve).
  afv_lba.hip         in: cams, slots, ids, the three edge arrays, pt_ptr, kf_ptr, kf_edge, (GBA) col_ptr / blk_row / blk_col / blk_kind - every
                      index the kernels follow.  zero: LbStatus.  scratch: e_state, kf_out, xyz_out (read back) and the take() regions
                      (cam, obs, stereo, e_on, e_chi2, p_on, pose, xyz, term, rho, Hll, Hinv, Hpp, M | L, bS, dx, p_fail, k_fail: values and
                      flag BYTES, no index among them; k_lba_gather is the first launch); solve_fail is filled with 0 on the stream.
                      afv_points_correct_se3: in ids, pairs, transforms; scratch: the status bytes, written per id and fetched.
  afv_essgraph.hip    in: S, fixed, v0, v1, measurements, ids, ref.  zero: EgStatus.  scratch: S_out, Tiw, xyz, status (read back), take():
                      Swc, perturbations, errors, terms, Hd, A, L, rhs, chi, e_bad / v_fail (flag bytes), solve_fail.
                      afv_points_correct_sim3: as correct_se3.
  afv_refresh.hip     in: slots, centres, kf_bad (or zero), point ids, ref_kf, the observation arrays.  scratch: status, best, med (filled on the
                      stream where a part is switched off), crow / cobs (row and observation lists k_refresh_desc writes before it reads).
  afv_triangulate.hip in: jobs, pairs, match12.  scratch: status, route, x3d, new_id, n_new, block counts, total - written by the count pass
                      before the scan reads them; fetched.
  afv_newpoints.hip   in: geometry jobs, masks.  zero: the search jobs, next / stop words.  scratch: match12 (the search kernel writes every
                      row before the triangulation reads it), status, route, x3d, new_id, n_new, block counts.
  afv_kffuse.hip      in: ids, poses.  zero: fuse jobs, projection jobs, grid jobs.  scratch: gathered rows, the six query planes and the
                      valid bytes (k_points_project), best / occupant / status (the search kernel; fetched).
  afv_points.hip      afv_frame_project_points / the searches through ids: in ids; scratch: the query planes, valid, occupies, count - all
                      written by k_points_project, which leaves d_points_count = {0, 0} behind its last workgroup.
  afv_project.hip     in: every query plane, rows, occupied bytes, reference slots.  zero: DevProjJob / DevGridJob records, nmatches.  scratch:
                      keys, ncand, orilist (phase 1 writes a query's record before phase 2 reads it), cell_ptr / cell_ent (k_frame_grid, launched
                      first when the side is staged), the output row.  The records hold addresses: the staging loop stages again after a growth.
  afv_match_jobs.hip  in: rows, idx, valid, angles, segments, tasks.  zero: job records, histograms, nmatches.  scratch: the output rows (filled
                      with -1 on the stream), the orientation bins.  afv_match_bow_plain32: zero rows / counts / pairs / angles are uploaded; the
                      match rows and nmatches are NOT (the upload ends before them): the resolve kernel writes every row and count.
  afv_stereo.hip      afv_frame_set_depth: in the depth image (the whole of what it lays into d_match); the kernel writes the frame's own
                      planes.  afv_frame_stereo_match works in the planes and pyramids of the two frames; it does not touch d_match.
  afv_comm.hip        afv_table_score_bow: in queries (zero records), scratch: score / common / first - written for every (query, slot) cell.
                      afv_table_match_pairs: the table's own d_pairs / d_out / d_nm / h_pin (painted too).
  afv_api.hip         afv_match_l2: in rows, valid; zero: the output row and count; scratch: the key records.  afv_bow_vector: in leaves;
                      scratch: n, word, value.  afv_bow_transform*: in rows; zero: leaf, node.  afv_distinctive_descriptors*: in rows, set_ptr;
                      zero: best index, best median.  The pair matchers: d_topk / d_slice / d_l2_scratch are key records phase 1 writes and
                      phase 2 reads; d_tickets are zero at rest.
  afv_extract.hip     afv_orb_compute: in the keypoints; the descriptors come back through d_match.
The lines above come from the layout code of each host file and the order of its launches; the kernels were read through where a later
launch follows a scratch region as an index or a count (k_newpoints.hip and k_triangulate.hip: match12, status and the block counts are
written for every lane below cap before the store launch reads them; k_lba.hip's indices are all inputs).  This reading found no region
read before it is written.  What it cannot show - a kernel that reads beyond the part an earlier one wrote - is what the painted runs
are for."""
import contextlib
import importlib
import inspect

import numpy as np

CTX = dict(max_width=640, max_height=480, max_batch=1)   # the default geometry: what the scenes of the reused modules are extracted at


class Case:
    def __init__(self, name, entries, make, ctx=None, holds=()):
        """holds: "points" / "tables" - the row keeps a store / a table with pair buffers alive across the passes"""
        self.name, self.entries, self.make, self.ctx, self.holds = name, tuple(entries), make, dict(CTX, **(ctx or {})), tuple(holds)

    def __repr__(self):
        return self.name


def matcher_for(afv, ctx):
    """the `matcher` fixture of test_gpu_match.py on another context"""
    afv.FeatureMatcher.setDescriptorDistanceThresholds({"FeatureMatcher.matchingTh": 75.0})
    return afv.FeatureMatcher(0.6, True, ctx=ctx)


def reuse(module, function, **params):
    """make() of a row whose step is the test `function` of tests/`module`.py, the fresh context in the place of every context fixture"""
    def make(afv, ctx, oracle):
        fn = getattr(importlib.import_module(module), function)
        fixtures = dict(afv=afv, oracle=oracle, gpu_ctx=ctx, fctx=ctx, sctx=ctx, tbl=afv.table, pairs_path="batch-kernels")
        names = list(inspect.signature(fn).parameters)
        missing = [n for n in names if n not in fixtures and n not in params and n != "matcher"]
        assert not missing, (module, function, missing)

        def step():
            kw = {n: fixtures[n] for n in names if n in fixtures}
            if "matcher" in names:
                kw["matcher"] = matcher_for(afv, ctx)
            kw.update(params)
            fn(**kw)
        return step
    make.reused = (module, function, params)
    return make


# ---- rows with a step of their own: the module's rig and expected answer, where its test function makes contexts of its own ----
def pose_rig(afv, ctx):
    import _poseopt_scenes as S
    from test_gpu_poseopt import Rig
    s = S.random_scene(65 % 7, 65, "mixed")
    return s, Rig(afv, ctx, s)


def make_pose_optimize(afv, ctx, oracle):
    """the rig lives across the passes: every step writes the store again through its (painted) staging, then optimises"""
    from test_gpu_poseopt import assert_equal
    s, rig = pose_rig(afv, ctx)
    ids = np.flatnonzero(s.store_set)

    def step():
        rig.points.set(ids, pos=s.store_pos[ids])
        assert_equal(rig.frame.PoseOptimizationBatch(rig.points, [s.pts])[0], s.run(inf=rig.inf), "pose_optimize")
    step.close = rig.close
    return step


def make_points_setters(afv, ctx, oracle):
    """a store that lives across the passes: every setter of it and afv_points_get through its own staging (d_stage / h_pin), what comes
    back against what went in, bit for bit"""
    import _points_ref as PR
    import test_gpu_points as T
    P = T.random_scene(0, PR.FRUSTUM).P
    points = afv.MapPoints(ctx, P.capacity, desc_bytes=P.desc_bytes, float_dim=P.float_dim)
    ids = np.flatnonzero(P.flags & PR.SET).astype(np.int32)
    rest = np.flatnonzero((P.flags & PR.SET) == 0).astype(np.int32)

    def step():
        T.fill_store(points, P)
        g = points.get(ids)
        for k in ("pos", "normal", "min_distance", "max_distance", "ref_size", "ref_distance", "ref_sigma", "descriptors"):
            want = np.ascontiguousarray(getattr(P, k)[ids], g[k].dtype)
            assert g[k].shape == want.shape and g[k].tobytes() == want.tobytes(), k
        assert np.array_equal(g["flags"] & 7, P.flags[ids] & 7), "flags"
        if len(rest):
            assert not (points.get(rest)["flags"] & PR.SET).any(), "an id that was never set"
    step.close = points.close
    return step


def make_bundle_adjust(module, rig_name, scenes_name, want_name, scene):
    """a bundle adjustment whose table and store live across the passes; the call moves the points, so every step first writes the
    scene's positions again through the store's (painted) staging"""
    def make(afv, ctx, oracle):
        T = importlib.import_module(module)
        from test_gpu_lba import assert_equal
        sc = getattr(T, scenes_name)[scene]
        want = getattr(T, want_name)(scene, sc)
        rig = getattr(T, rig_name)(afv, ctx, sc)
        ok = np.nonzero(sc.p_ok)[0]

        def step():
            if len(ok):
                rig.points.set(sc.ids[ok], pos=sc.pos[ok])
            code, res, kf, xyz, state = rig.call()
            assert code == 0, scene
            assert_equal((res, kf, xyz, state), want, scene)
        step.close = rig.close
        return step
    return make


def make_table_fuse_points(afv, ctx, oracle):
    """test_gpu_kffuse.py::run_map with the rig alive across the passes (the call writes neither store nor planes); the store is written
    again through its staging in every step"""
    import _kffuse_scenes as KS
    import test_gpu_kffuse as T
    m = T.the_map(1, 63, 65, 7)
    rig = T.Rig(afv, ctx, m.P, m.kfs, m.grid)
    jobs = [dict(slot=k, ids=m.lists[k], th_low=m.th_low, use_inf_gate=True, pose=None) for k in sorted(m.kfs)]

    def step():
        T.fill_store(rig.points, m.P)
        T.assert_same(T.call(rig, jobs), KS.expected(m, True, None), m.name)
    step.close = rig.close
    return step


def make_table_match_pairs(afv, ctx, oracle):
    """afv_table_match_pairs on a table that lives across the passes: its d_pairs / d_out / d_nm / h_pin are painted between the calls"""
    import test_gpu_table as T
    table, host, _, _ = small_table(afv, ctx)
    pa = np.array([0, 1, 2, 3, 4, 6, 7, 5, 0], np.int32)
    pb = np.array([1, 2, 3, 4, 6, 7, 0, 1, 5], np.int32)

    def step():
        m, nm = table.match_pairs(pa, pb, T.TH, T.RATIO, True)
        for j in range(len(pa)):
            want, wn = T._oracle_job(oracle, host, int(pa[j]), int(pb[j]))
            assert nm[j] == wn and np.array_equal(m[j, :host[2][pa[j]]], want) and (m[j, host[2][pa[j]]:] == -1).all(), j
        _, counts = table.match_pairs(pa, pb, T.TH, T.RATIO, True, want_matches=False)
        assert np.array_equal(counts, nm) and nm.sum() > 50
    step.close = table.close
    return step


def make_frame_match_initialization(afv, ctx, oracle):
    """test_gpu_frame.py::test_initialization_between_two_resident_frames (seed 24, shift 6, window 100) on the given context"""
    def step():
        img = afv.synth.corners_frame(24)
        f1, f2 = afv.Frame(ctx), afv.Frame(ctx)
        try:
            k1, d1 = f1.extract(img)
            k2, d2 = f2.extract(np.roll(img, 6, axis=1))
            z2 = ctx.size_sigma(k2)[0]
            F2 = afv.FrameGridView(d2, np.stack([k2["x"], k2["y"]], 1), z2, angles=k2["angle"])
            prev = np.stack([k1["x"], k1["y"]], 1).astype(np.float32)
            n1 = len(k1)
            maxsz = np.float32(max(ctx.size_sigma(np.array([(0, 0, 0, 0, 0, o, -1)], afv.KP_DTYPE))[0][0] for o in range(8)))
            Q1 = afv.ProjectionQueries(d1, prev[:, 0].copy(), prev[:, 1].copy(), np.full(n1, 100.0, np.float32), np.zeros(n1, np.float32),
                                       np.full(n1, maxsz, np.float32), valid=(k1["octave"] == 0).astype(np.uint8), angles=k1["angle"])
            afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)
            got, n = f1.SearchForInitialization(afv.FeatureMatcher(0.9, True, ctx=ctx), f2, prev, windowSize=100.0)
            want, wn = oracle.match_initialization(F2, Q1, th_low=75.0, nnratio=0.9, check_orientation=True)
            assert n == wn and np.array_equal(got, want) and wn > 50
        finally:
            f1.close(); f2.close()
    return step


def small_table(afv, ctx):
    """test_gpu_table.py's ragged table (8 keyframes of up to 128 rows, one empty) with FeatureVectors and validity masks"""
    import test_gpu_table as T
    t, ang, cnt = T._small_table(afv, K=8, cap=128)
    table = afv.table.DescriptorTable(ctx, len(cnt), t.shape[1])
    fvs, valid = [], [None] * len(cnt)
    for k in range(len(cnt)):
        table.set(k, t[k, :cnt[k]], ang[k, :cnt[k]])
        fvs.append(T._featvec(afv, 77, int(cnt[k]), 12 if k % 4 else 5))
        table.set_featvec(k, *T._csr(fvs[k]))
        if k % 3 == 0 and cnt[k]:
            valid[k] = (afv.synth.lcg_bytes(900 + k, int(cnt[k])) > 50).astype(np.uint8)
            table.set_valid(k, valid[k])
    return table, (t, ang, cnt), fvs, valid


def make_table_match_bow_frame(afv, ctx, oracle):
    """test_gpu_table.py::test_table_bow_frame_relocalisation_batch at 8 keyframes, on the given context"""
    import test_gpu_table as T

    def step():
        table, (t, ang, cnt), fvs, valid = small_table(afv, ctx)
        try:
            nf = 100
            fdesc = afv.synth.perturbed_descriptors(t[3, :nf].copy(), 4242)
            fang = ((ang[3, :nf] + 3.0) % 360.0).astype(np.float32)
            ffv = T._featvec(afv, 77, nf, 12)
            slots = np.arange(len(cnt), dtype=np.int32)[::-1].copy()
            m, nm = table.match_bow_frame(slots, afv.FeatureView(fdesc, ffv, None, fang), T.TH, T.RATIO, True)
            total = 0
            for p, k in enumerate(slots):
                want, wn = oracle.search_by_bow_kf_frame(t[k, :cnt[k]], fdesc, fvs[k], ffv, valid[k], ang[k, :cnt[k]], fang, T.TH, T.RATIO, True)
                assert nm[p] == wn and np.array_equal(m[p], want), (p, k)
                total += wn
            assert total > 50
        finally:
            table.close()
    return step


def make_table_match_pairs_device(afv, ctx, oracle):
    """the device-pointer pair call of test_gpu_table.py::test_config4_full_size_10k_jobs at 8 keyframes, every job against the oracle"""
    import torch
    import test_gpu_table as T

    def step():
        table, host, _, _ = small_table(afv, ctx)
        try:
            pa = np.array([0, 1, 2, 3, 4, 6, 7, 5, 0], np.int32)
            pb = np.array([1, 2, 3, 4, 6, 7, 0, 1, 5], np.int32)
            match, nm = table.match_pairs_device(torch.from_numpy(pa).cuda(), torch.from_numpy(pb).cuda(), T.TH, T.RATIO, True)
            torch.cuda.synchronize()
            match, nm = match.cpu().numpy(), nm.cpu().numpy()
            cnt = host[2]
            for j in range(len(pa)):
                want, wn = T._oracle_job(oracle, host, int(pa[j]), int(pb[j]))
                assert nm[j] == wn and np.array_equal(match[j, :cnt[pa[j]]], want), j
            assert nm.sum() > 50
        finally:
            table.close()
    return step


def make_orb_compute(afv, ctx, oracle):
    """test_gpu_extract.py::test_detect_then_compute_is_extract on the given context"""
    def step():
        img = afv.synth.corners_frame(1)
        k, d = ctx.extract(img)
        kd = ctx.detect(img)
        assert kd.tobytes() == k.tobytes() and len(k) > 900
        got = ctx.compute(img, kd)
        assert np.array_equal(got, d) and np.array_equal(got, oracle.orb_compute(img, kd))
    return step


def stereo_ctx():
    import _stereo_scenes as SS
    return dict(nfeatures=300, nlevels=SS.NLEVELS, scale_factor=SS.SCALE, max_width=SS.WIDTH, max_height=SS.HEIGHT)


def stereo_scene(name):
    import _stereo_scenes as SS
    return next(s for s in SS.all_scenes() if s.name == name)


def make_stereo_match(afv, ctx, oracle):
    import test_gpu_stereo as T

    def step():
        for name in ("sizes_N65_Nr63", "rows_32_bytes"):
            T.test_scene_against_the_restatement(afv, ctx, stereo_scene(name))
    return step


def _cases():
    import _points_ref as PR
    import _refresh_scenes as RS
    import _voctrain_scenes as VS
    rows = [
        Case("frame_pose_optimize", ["afv_frame_pose_optimize", "afv_points_set"], make_pose_optimize, holds=["points"]),
        Case("points_setters", ["afv_points_set", "afv_points_set_flags", "afv_points_set_descriptors", "afv_points_get"], make_points_setters,
             holds=["points"]),
        Case("table_match_pairs", ["afv_table_match_pairs"], make_table_match_pairs, holds=["tables"]),
        Case("table_fuse_points_kept_rig", ["afv_table_fuse_points", "afv_points_set", "afv_points_set_flags", "afv_points_set_descriptors"],
             make_table_fuse_points, holds=["points"]),
        Case("table_bundle_adjust_kept_rig", ["afv_table_bundle_adjust", "afv_points_set"],
             make_bundle_adjust("test_gpu_lba", "Rig", "SCENES", "want_ref", "mixed_mono_stereo"), holds=["points"]),
        Case("table_global_bundle_adjust_kept_rig", ["afv_table_global_bundle_adjust", "afv_points_set"],
             make_bundle_adjust("test_gpu_gba", "GRig", "SMALL", "want_sparse", "pattern_empties"), holds=["points"]),
        Case("frame_pnp_hypotheses", ["afv_frame_pnp_hypotheses"], reuse("test_gpu_pnp", "test_correspondence_counts", n=65)),
        Case("frame_initializer", ["afv_frame_initializer"], reuse("test_gpu_init", "test_scene_is_bit_equal_to_the_restatement", name="n65")),
        Case("frame_search_points", ["afv_frame_search_points", "afv_frame_project_points", "afv_frame_match_projection"],
             reuse("test_gpu_points", "test_random_scene_projection_and_search", seed=0, fl=PR.FRUSTUM)),
        Case("frame_search_points_last_frame", ["afv_frame_search_points", "afv_frame_project_points"],
             reuse("test_gpu_points", "test_random_scene_projection_and_search", seed=1, fl=PR.LASTFRAME)),
        Case("frame_fuse_points", ["afv_frame_fuse_points", "afv_frame_match_fuse"],
             reuse("test_gpu_points", "test_random_scene_projection_and_search", seed=0, fl=PR.FUSE)),
        Case("frame_match_fuse", ["afv_frame_match_fuse"], reuse("test_gpu_frame", "test_fuse_on_a_resident_frame")),
        # the three engines of the ordered phase; 1 is the one-launch search that hands over through d_proj_ticket
        Case("frame_match_projection_one_launch", ["afv_frame_match_projection", "afv_match_projection"],
             reuse("test_gpu_frame", "test_projection_searches_on_the_resident_frame", seed=5, shift=5, rs=15.0, last=True, engine=1)),
        Case("frame_match_projection_two_launches", ["afv_frame_match_projection", "afv_match_projection"],
             reuse("test_gpu_frame", "test_projection_searches_on_the_resident_frame", seed=1, shift=4, rs=15.0, last=False, engine=3)),
        Case("frame_match_projection_ordered_walk", ["afv_frame_match_projection", "afv_match_projection"],
             reuse("test_gpu_frame", "test_projection_searches_on_the_resident_frame", seed=5, shift=5, rs=15.0, last=True, engine=0)),
        Case("frame_match_initialization", ["afv_frame_match_initialization"], make_frame_match_initialization),
        Case("frame_stereo_match", ["afv_frame_stereo_match"], make_stereo_match, ctx=stereo_ctx()),
        Case("frame_set_depth", ["afv_frame_set_depth"], reuse("test_gpu_stereo", "test_rgbd_gather"), ctx=stereo_ctx()),
        Case("frame_bow_transform", ["afv_frame_bow_transform", "afv_bow_vector"],
             reuse("test_gpu_bowvec", "test_stopped_words_and_repeated_addition")),
        Case("match_projection", ["afv_match_projection"], reuse("test_gpu_projection", "test_last_frame_mode", seed=5, shift=5, rs=15.0, ori=True)),
        Case("match_fuse", ["afv_match_fuse"], reuse("test_gpu_projection", "test_fuse_core", seed=11, shift=4, rs=15.0)),
        Case("match_sim3", ["afv_match_sim3"], reuse("test_gpu_projection", "test_search_by_sim3")),
        Case("match_initialization", ["afv_match_initialization"],
             reuse("test_gpu_projection", "test_search_for_initialization", seed=24, shift=6, window=100.0, ori=True)),
        Case("match_bow", ["afv_match_bow"], reuse("test_gpu_match", "test_bow_guided_with_validity", frame=False)),
        Case("match_bow_plain", ["afv_match_bow"], reuse("test_gpu_match", "test_batch_of_jobs")),
        Case("match_triangulation", ["afv_match_triangulation"], reuse("test_gpu_match", "test_triangulation")),
        Case("match_l2", ["afv_match_l2"], reuse("test_gpu_match", "test_l2_float_descriptors")),
        Case("match_l2_pairs_device", ["afv_match_l2_pairs_device"],
             reuse("test_gpu_match", "test_l2_pairs_in_several_launches_with_a_ragged_last_one")),
        Case("match_bruteforce_pairs_device", ["afv_match_bruteforce_pairs_device"],
             reuse("test_gpu_match", "test_device_pairs_match_extracted_frames"), ctx=dict(max_batch=4)),
        Case("bow_transform", ["afv_bow_transform"], reuse("test_gpu_bow", "test_transform_nodes_match_oracle", k=6, L=3, levelsup=1)),
        Case("bow_transform_f32", ["afv_bow_transform_f32"], reuse("test_gpu_bow", "test_float_vocabulary_descent", dim=64, k=10, L=3, levelsup=2)),
        Case("bow_vector", ["afv_bow_vector"], reuse("test_gpu_bowvec", "test_frame_bowvec_equals_the_restatement", kind="orb32")),
        Case("distinctive_descriptors", ["afv_distinctive_descriptors"],
             reuse("test_gpu_match", "test_distinctive_descriptors_of_map_points", nbytes=32)),
        Case("distinctive_descriptors_f32", ["afv_distinctive_descriptors_f32"],
             reuse("test_gpu_match", "test_distinctive_descriptors_of_float_map_points", dim=64, real=False)),
        Case("table_matchers_on_promoted_frames",
             ["afv_table_match_pairs", "afv_table_match_bow", "afv_table_match_bow_frame_h", "afv_table_match_triangulation", "afv_frame_bow_transform",
              "afv_bow_transform"], reuse("test_gpu_frame", "test_compute_bow_on_the_frame_and_search_by_bow")),
        Case("table_match_bow_frame", ["afv_table_match_bow_frame"], make_table_match_bow_frame),
        Case("table_match_pairs_device", ["afv_table_match_pairs_device"], make_table_match_pairs_device),
        Case("table_score_bow", ["afv_table_score_bow"],
             reuse("test_gpu_table_bow", "test_scores_equal_the_restatement_for_every_query_kind", kind="orb32")),
        Case("table_triangulate", ["afv_table_triangulate"], reuse("test_gpu_triangulate", "test_random_scenes", kind="both_stereo", seed=0)),
        Case("table_create_new_points", ["afv_table_create_new_points", "afv_table_match_triangulation", "afv_table_triangulate"],
             reuse("test_gpu_newpts_chain", "test_rows_equal_the_restatement_and_the_existing_loop", key=(1, 3, 40, 32, 0))),
        Case("table_fuse_points", ["afv_table_fuse_points"], reuse("test_gpu_kffuse", "test_random_map_shapes", nq=63, nf=65, nt=7)),
        Case("table_sim3_hypotheses", ["afv_table_sim3_hypotheses"], reuse("test_gpu_sim3", "test_correspondence_counts_at_the_edges", n=65)),
        Case("table_optimize_sim3", ["afv_table_optimize_sim3"], reuse("test_gpu_sim3opt", "test_correspondence_counts_at_the_edges", n=65)),
        Case("table_bundle_adjust", ["afv_table_bundle_adjust"],
             reuse("test_gpu_lba", "test_every_constructed_scene_against_the_restatement", name="mixed_mono_stereo")),
        Case("table_bundle_adjust_bad_pivot", ["afv_table_bundle_adjust"],
             reuse("test_gpu_lba", "test_every_constructed_scene_against_the_restatement", name="bad_pivot")),
        Case("table_global_bundle_adjust", ["afv_table_global_bundle_adjust"],
             reuse("test_gpu_gba", "test_every_small_scene_against_the_sparse_restatement", name="pattern_empties")),
        Case("table_refresh_points", ["afv_table_refresh_points"],
             reuse("test_gpu_refresh", "test_every_rule_against_the_restatement", kind=RS.KINDS[0], parts="both")),
        Case("essential_graph", ["afv_essential_graph"],
             reuse("test_gpu_essgraph", "test_constructed_scene_is_bit_equal_to_the_restatement", name="drifted_loop")),
        Case("points_correct_sim3", ["afv_points_correct_sim3", "afv_essential_graph"],
             reuse("test_gpu_essgraph", "test_point_correction_through_both_entries", npts=65, kind="binary")),
        Case("points_correct_se3", ["afv_points_correct_se3"], reuse("test_gpu_gba", "test_correct_se3_against_the_restatement", n=65, m=7)),
        Case("orb_compute", ["afv_orb_compute"], make_orb_compute),
        Case("vocab_train", ["afv_vocab_train"], reuse("test_gpu_voctrain", "test_scene_bit_equal", sc=VS.by_name("shape_k3_L2_b61"), entry="host")),
    ]
    assert len({r.name for r in rows}) == len(rows)
    return rows


CASES = _cases()
# called by every row: the test closes its fresh context while the recorder is on, and afv_destroy frees the painted buffers
EVERY_ROW = ("afv_destroy",)


def covered():
    return {e for r in CASES for e in r.entries} | set(EVERY_ROW)


# ---- every other declaration of include/afv_hip.h, each with the reason it has no row.  tests/test_scratch_cases_cpu.py refuses an entry
#      here whose body in csrc/ mentions d_match, Blob or ensure_match_buffer ----
_LEFT_OUT = {
    "creates, destroys or clones an object; no per-call scratch": [
        "afv_create", "afv_frame_create", "afv_frame_destroy", "afv_points_create", "afv_points_destroy", "afv_table_create", "afv_table_create_bytes",
        "afv_table_create_f32", "afv_table_destroy", "afv_table_clone", "afv_vocab_create", "afv_vocab_create_f32", "afv_vocab_destroy",
        "afv_vocab_tree_destroy", "afv_comm_create", "afv_comm_destroy"],
    "host only: no device work, no context scratch": [
        "afv_abi_version", "afv_default_orb_params", "afv_strerror", "afv_last_error", "afv_stream", "afv_hamming256", "afv_num_stages",
        "afv_get_geometry", "afv_max_keypoints_per_frame", "afv_orb_size_sigma", "afv_pyramid_level_sizes", "afv_shard_range", "afv_frame_count",
        "afv_frame_device_ptrs", "afv_table_device_ptrs", "afv_gba_plan_probe", "afv_debug_pyramid_plan", "afv_debug_fast_tiles",
        "afv_debug_describe_reach", "afv_vocab_tree_nnodes", "afv_vocab_tree_get", "afv_vocab_tree_stats", "afv_comm_rank", "afv_comm_size",
        "afv_comm_unique_id", "afv_profile_enable", "afv_profile_read"],
    "a setting of the context; no kernel": [
        "afv_set_l2_chunk_pairs", "afv_set_match_engine", "afv_set_match_resolve", "afv_set_pipeline_chunk", "afv_set_projection_resolve",
        "afv_set_small_batch_path", "afv_set_split_chunks", "afv_set_split_schedule", "afv_set_split_threshold"],
    "the hooks of this test": ["afv_debug_scratch_bytes", "afv_debug_paint_scratch", "afv_debug_rest_words", "afv_debug_scratch_read"],
    "the extraction pipeline works in the working set sized at afv_create, which is not painted (the getters read the last extraction out of it); "
    "tests/test_gpu_extract*.py and test_gpu_detect_scenes.py compare it stage by stage; the rows that extract run it on fresh contexts": [
        "afv_orb_extract", "afv_orb_detect", "afv_orb_extract_batch", "afv_orb_extract_batch_device", "afv_frame_extract", "afv_debug_get_level",
        "afv_debug_get_candidates", "afv_debug_get_selected", "afv_debug_blur_level"],
    "setter or getter of resident planes: copies into or out of the object's own planes, never through d_match (the store's setters and "
    "afv_points_get, which stage through the store's d_stage / h_pin, have rows that keep the store alive across the paints; afv_points_set_descriptors_from_table stages its three index arrays the same "
    "way and has none: tests/test_gpu_points.py compares it with the host-row setter)": [
        "afv_frame_set_features", "afv_frame_set_pose", "afv_frame_set_pyramid", "afv_frame_set_undistorted", "afv_frame_get_bowvec",
        "afv_frame_get_featvec", "afv_frame_get_grid", "afv_frame_get_pyramid_level", "afv_frame_get_stereo",
        "afv_points_set_descriptors_from_table", "afv_table_set", "afv_table_set_bowvec",
        "afv_table_set_camera", "afv_table_set_featvec", "afv_table_set_from_frame", "afv_table_set_geometry", "afv_table_set_inf",
        "afv_table_set_map_points", "afv_table_get_map_points", "afv_table_set_pose", "afv_table_set_scale", "afv_table_set_u_right",
        "afv_table_set_valid", "afv_table_sync_counts", "afv_vocab_set_stopped", "afv_vocab_set_weights"],
    "needs several GPUs or ranks (tests/test_gpu_table.py::test_comm_two_ranks)": ["afv_table_broadcast", "afv_comm_allgather", "afv_comm_broadcast"],
    "trains on rows the caller keeps on the device, in buffers of its own; the host-row entry afv_vocab_train has a row": ["afv_vocab_train_device"],
}
LEFT_OUT = {name: reason for reason, names in _LEFT_OUT.items() for name in names}
assert sum(len(v) for v in _LEFT_OUT.values()) == len(LEFT_OUT), "an entry point is left out twice"


@contextlib.contextmanager
def recording(lib, symbols):
    """while the block runs, every call of a declared symbol of the loaded library is noted: yields the set of names"""
    called, saved = set(), {}
    for name in symbols:
        fn = getattr(lib, name)
        saved[name] = fn

        def wrapper(*a, _fn=fn, _name=name):
            called.add(_name)
            return _fn(*a)
        setattr(lib, name, wrapper)
    try:
        yield called
    finally:
        for name, fn in saved.items():
            setattr(lib, name, fn)


# ---- the role chains: what one thread of a SLAM host alternates over the same bytes.  A step builds the rig of its module on the
#      given context, makes the call, holds the answer to the module's restatement and returns the answer as bytes; no step takes
#      anything from the step before (calls that feed each other sit inside one step: step_search_optimise_search), so a step alone
#      on a fresh context gives the bytes every other run must repeat ----
def to_bytes(x):
    """an answer of any of the wrappers as bytes: arrays with dtype and shape, containers in order (dicts by key), ctypes records raw"""
    import ctypes
    if isinstance(x, np.ndarray):
        return ("%s%s" % (x.dtype.str, x.shape)).encode() + np.ascontiguousarray(x).tobytes()
    if isinstance(x, dict):
        return b"{" + b"".join(repr(k).encode() + b":" + to_bytes(x[k]) for k in sorted(x, key=repr)) + b"}"
    if isinstance(x, (list, tuple)):
        return b"[" + b",".join(to_bytes(v) for v in x) + b"]"
    if isinstance(x, (ctypes.Structure, ctypes.Array)):
        return bytes(x)
    if isinstance(x, (bytes, bytearray)):
        return bytes(x)
    if isinstance(x, (float, np.floating)):
        return np.float64(x).tobytes()
    if x is None or isinstance(x, (bool, int, str, np.integer, np.bool_)):
        return repr(x).encode()
    raise TypeError(type(x))


def store_bytes(points):
    return to_bytes(points.get(np.arange(points.capacity, dtype=np.int32)))


def step_compute_bow(afv, ctx, oracle):
    """set_features + ComputeBoW: the frame's leaves and its BowVector against the restatement of DBoW2's transform"""
    import _kfdb_ref as ref
    from test_gpu_bowvec import _frame, _same
    voc = afv.Vocabulary.random(3, ctx=ctx)
    fr = _frame(afv, ctx, "orb32", afv.synth.random_descriptors(9, 300), cap=300)
    try:
        leaf, nid = fr.bow_transform_nodes(voc)
        oleaf, onid = oracle.bow_transform(voc, afv.synth.random_descriptors(9, 300), 4)
        assert np.array_equal(leaf, oleaf)
        _same(fr.bowvec(), ref.bow_vector(leaf, voc.weight, voc.word_id))
        return to_bytes([leaf, nid, fr.bowvec()])
    finally:
        fr.close(); voc.close()


def _points_search(afv, ctx, seed, flavour):
    import test_gpu_points as T
    s = T.random_scene(seed, flavour)
    rig = T.Rig(afv, ctx, s)
    try:
        got = rig.search()
        T.check_search(afv, rig, s)
        return to_bytes([got, rig.project()])
    finally:
        rig.close()


def step_search_local_points(afv, ctx, oracle):
    import _points_ref as PR
    return _points_search(afv, ctx, 0, PR.FRUSTUM)


def step_search_by_projection_last(afv, ctx, oracle):
    import _points_ref as PR
    return _points_search(afv, ctx, 1, PR.LASTFRAME)


def _pose_optimization(afv, ctx, seed, n, kind):
    import _poseopt_scenes as S
    from test_gpu_poseopt import Rig, assert_equal
    s = S.random_scene(seed, n, kind)
    rig = Rig(afv, ctx, s)
    try:
        got = rig.frame.PoseOptimizationBatch(rig.points, [s.pts])[0]
        assert_equal(got, s.run(inf=rig.inf), ("chain", n, kind))
        return to_bytes(got)
    finally:
        rig.close()


def step_pose_optimization(afv, ctx, oracle):
    return _pose_optimization(afv, ctx, 65 % 7, 65, "mixed")


def step_pose_optimization_again(afv, ctx, oracle):
    return _pose_optimization(afv, ctx, 63 % 7, 63, "stereo")


def step_pose_optimization_large(afv, ctx, oracle):
    return _pose_optimization(afv, ctx, 1025 % 7, 1025, "mixed")


def step_search_optimise_search(afv, ctx, oracle):
    """the one step whose calls feed each other (test_gpu_poseopt.py::test_chain_search_optimise_search, the pose staying in the
    library): SearchLocalPoints -> PoseOptimization on its matches -> SearchLocalPoints under the new pose.  Held to the other runs'
    bytes, not to a restatement"""
    import _points_ref as PR
    import _points_scenes as PS
    from test_gpu_points import fill_store
    ps = PS.random_scene(1, PR.FRUSTUM)
    P, cam, f = ps.P, ps.cam, ps.feat
    points = afv.MapPoints(ctx, P.capacity, desc_bytes=P.desc_bytes)
    frame = afv.Frame(ctx, max_x=PS.W, max_y=PS.H, cap=f.n)
    try:
        fill_store(points, P)
        kps = np.zeros(f.n, afv.KP_DTYPE)
        kps["x"], kps["y"], kps["angle"] = f.x, f.y, f.angles
        frame.set_features(kps, f.desc, sizes=f.sizes, u_right=f.u_right)
        frame.set_pose(cam.Rcw, cam.tcw, cam.Ow, cam.fx, cam.fy, cam.cx, cam.cy, cam.mbf)
        afv.FeatureMatcher.setDescriptorDistanceThresholds(ps.th)
        m = afv.FeatureMatcher(ps.nnratio, False, ctx=ctx)
        a1, n1, _ = frame.SearchLocalPoints(m, points, ps.ids, ps.radius_th, ps.cos_limit)
        pts = np.where(a1 >= 0, np.asarray(ps.ids)[np.clip(a1, 0, None)], -1).astype(np.int32)
        ng, outl, Tcw = frame.PoseOptimization(points, pts)
        a2, n2, iv2 = frame.SearchLocalPoints(m, points, ps.ids, ps.radius_th, ps.cos_limit)
        assert n1 >= 5 and ng >= 3
        return to_bytes([a1, n1, ng, outl, Tcw, a2, n2, iv2])
    finally:
        afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)
        frame.close()
        points.close()


def step_pnp_solver_batch(afv, ctx, oracle):
    import _pnp_scenes as S
    import test_gpu_pnp as T
    s = S.build("n65", 65, 65, 65 // 5, 100 + 65, octaves=True, min_inliers=4, epsilon=0.3, nhyp=8)
    r = T.Rig(afv, ctx, s)
    try:
        got = r.call()
        for c in range(s.nc):
            T.assert_candidate(got, c, s.run(c, r.sigma2, None, None), ("chain", c))
        return to_bytes(got)
    finally:
        r.close()


def step_create_new_map_points_chain(afv, ctx, oracle):
    import _newpts_scenes as N
    import test_gpu_newpts_chain as T
    key = (1, 3, 40, 32, 0)
    ch = N.chain(*key)
    nbs, cams, F12, ep = T.call_args(ch)
    pts, before = T.store_for(afv, ctx, ch)
    t = None
    try:
        t = T.build_table(afv, ctx, ch, T.CAPS[key])
        has_mp = T.mask_dict(ch)
        got = t.CreateNewMapPointsChain(pts, 0, nbs, cams, F12, ep, ch.th_low, has_mp, ch.first_id)
        assert got == T.observations(ch.want)
        T.assert_masks(ch, has_mp, ch.want, name=key)
        T.assert_store(pts, before, [(nid, k, i, f) for nid, k, i, j, f in ch.want], lambda p, i: ch.W.desc[0][i], key)
        return to_bytes([[list(o) for o in got], has_mp]) + store_bytes(pts)
    finally:
        pts.close()
        if t is not None:
            t.close()


def step_fuse_points(afv, ctx, oracle):
    """SearchInNeighbors: Fuse no. 1 (information gate) of a store into seven slots"""
    import test_gpu_kffuse as T
    return to_bytes(list(T.run_map(afv, ctx, T.the_map(1, 63, 65, 7))))   # run_map returns the expected answer the device's was equal to


def step_search_and_fuse(afv, ctx, oracle):
    """SearchAndFuse: Fuse no. 2 under a Sim3 pose per slot (test_gpu_kffuse.py::test_pose_override_sim3)"""
    import _kffuse_ref as K
    import test_gpu_kffuse as T
    m = T.the_map(4, 130, 90, 3, stereo=True)
    poses = {}
    for s, kf in m.kfs.items():
        Scw = np.eye(4, dtype=np.float32)
        Scw[:3, :3] = kf.cam.Rcw * np.float32(1.0 + 0.1 * s)
        Scw[:3, 3] = kf.cam.tcw
        poses[s] = K.decompose_scw(Scw)
    return to_bytes(list(T.run_map(afv, ctx, m, gate=False, poses=poses)))


def _bundle_adjustment(afv, ctx, rig_class, sc, want, name):
    from test_gpu_lba import assert_equal
    rig = rig_class(afv, ctx, sc)
    try:
        code, res, kf, xyz, state = rig.call()
        assert code == 0, name
        assert_equal((res, kf, xyz, state), want, name)
        return to_bytes([res, kf, xyz, state]) + store_bytes(rig.points)
    finally:
        rig.close()


def step_local_bundle_adjustment(afv, ctx, oracle):
    import test_gpu_lba as T
    return _bundle_adjustment(afv, ctx, T.Rig, T.SCENES["bad_pivot"], T.want_ref("bad_pivot", T.SCENES["bad_pivot"]), "bad_pivot")


def step_local_bundle_adjustment_large(afv, ctx, oracle):
    import test_gpu_lba as T
    return _bundle_adjustment(afv, ctx, T.Rig, T.SCENES["mixed_mono_stereo"], T.want_ref("mixed_mono_stereo", T.SCENES["mixed_mono_stereo"]), "mixed")


def step_global_bundle_adjustment(afv, ctx, oracle):
    import test_gpu_gba as T
    return _bundle_adjustment(afv, ctx, T.GRig, T.SMALL["bad_pivot"], T.want_sparse("bad_pivot", T.SMALL["bad_pivot"]), "gba bad_pivot")


def step_global_bundle_adjustment_large(afv, ctx, oracle):
    import test_gpu_gba as T
    return _bundle_adjustment(afv, ctx, T.GRig, T.SMALL["band"], T.want_sparse("band", T.SMALL["band"]), "gba band")


def step_refresh_after_bundle_adjustment(afv, ctx, oracle):
    import _refresh_scenes as RS
    import test_gpu_refresh as T
    sc, want = T.reference("rule_scene", RS.KINDS[0], (), (True, True))
    rig = T.Rig(afv, ctx, sc)
    try:
        status, best, med = rig.refresh(afv, True, True)
        assert np.array_equal(status, want[0]) and np.array_equal(best, want[1]) and med.tobytes() == want[2].tobytes()
        rig.assert_store(want[3], "chain")
        return to_bytes([status, best, med]) + store_bytes(rig.points)
    finally:
        rig.close()


def step_score_bow(afv, ctx, oracle):
    import _bow_scenes as scenes
    import test_gpu_table_bow as T
    s = scenes.scene("orb32")
    t, bows = T._fill(afv, ctx, "orb32", s)
    try:
        got = t.score_bow([7, s.loop_slot], None)
        for r, q in enumerate((7, s.loop_slot)):
            T._check([a[r] for a in got], T._want(bows[q], bows, s.nkf))
        return to_bytes(list(got))
    finally:
        t.close()


def step_match_bow(afv, ctx, oracle):
    import test_gpu_table as T
    table, (t, ang, cnt), fvs, valid = small_table(afv, ctx)
    try:
        pa = np.array([0, 1, 2, 3, 6, 7, 5], np.int32)
        pb = np.array([1, 2, 3, 4, 7, 0, 1], np.int32)
        m, nm = table.match_bow(pa, pb, T.TH, T.RATIO, True)
        for p in range(len(pa)):
            a, b = int(pa[p]), int(pb[p])
            want, wn = oracle.search_by_bow_kf_kf(t[a, :cnt[a]], t[b, :cnt[b]], fvs[a], fvs[b], valid[a], valid[b], ang[a, :cnt[a]], ang[b, :cnt[b]],
                                                  T.TH, T.RATIO, True)
            assert nm[p] == wn and np.array_equal(m[p, :cnt[a]], want), (p, a, b)
        return to_bytes([m, nm])
    finally:
        table.close()


def step_sim3_solver_batch(afv, ctx, oracle):
    import _sim3_scenes as S
    import test_gpu_sim3 as T
    sc = S.world(100 + 65, n=65, s=0.5, outliers=0.2, noise=0.4)
    sc.mp2[65:] = -1
    got, _ = T.run(afv, ctx, [sc], 288, 65, T.words_for(65), ("edges", 65))
    return to_bytes(got)


def step_optimize_sim3_batch(afv, ctx, oracle):
    import _sim3opt_scenes as S
    import test_gpu_sim3opt as T
    res, state = T.run(afv, ctx, [(("sized", 65), S.sized(65))], 320)
    return to_bytes([res, state])


def step_optimize_essential_graph(afv, ctx, oracle):
    import _essgraph_host as H
    import _essgraph_scenes as ES
    import test_gpu_essgraph as T
    sc, pr, want, _ = ES.solved("drifted_loop")
    pos, flags, ids, ref = ES.points_for(sc)
    pts = T.store_for(afv, ctx, pos, flags)
    try:
        code, res, S_out, Tiw, xyz, st = T.call(afv, ctx, sc, pts, ids, ref)
        assert code == 0
        T.assert_trace(res, want, "chain")
        assert S_out.tobytes() == H.records(want.S).tobytes() and Tiw.tobytes() == want.Tiw.tobytes()
        return to_bytes([res, S_out, Tiw, xyz, st]) + store_bytes(pts)
    finally:
        pts.close()


def step_correct_se3(afv, ctx, oracle):
    import _gba_ref as G
    from test_gpu_gba import seeded_transforms
    n, m = 65, 7
    rng = np.random.default_rng(100 + n)
    T = seeded_transforms(m, n)
    points = afv.MapPoints(ctx, 2 * n + 9)
    try:
        ids = rng.permutation(2 * n + 9)[:n].astype(np.int32)
        pos = rng.uniform(-8, 8, (n, 3)).astype(np.float32)
        pair = rng.integers(0, m, n).astype(np.int32)
        pair[[3, 7, 50]] = -1
        points.set(ids, pos=pos)
        before = points.get(ids)["pos"].copy()
        want, want_st = G.correct_se3(before, np.ones(n, bool), pair, T[0], T[1])
        st = points.correct_se3(ids, pair, T[0], T[1])
        assert np.array_equal(st, want_st) and points.get(ids)["pos"].tobytes() == want.tobytes()
        return to_bytes(st) + store_bytes(points)
    finally:
        points.close()


# name -> (the largest-footprint step on a larger scene of the same module, run once before the chain; the steps in order)
CHAINS = {
    "tracking": (step_pose_optimization_large,
                 [step_compute_bow, step_search_local_points, step_pose_optimization, step_search_by_projection_last, step_pnp_solver_batch,
                  step_pose_optimization_again, step_search_optimise_search]),
    "local_mapping": (step_local_bundle_adjustment_large,
                      [step_create_new_map_points_chain, step_fuse_points, step_local_bundle_adjustment, step_refresh_after_bundle_adjustment]),
    "loop_closing": (step_global_bundle_adjustment_large,
                     [step_score_bow, step_match_bow, step_sim3_solver_batch, step_optimize_sim3_batch, step_search_and_fuse,
                      step_optimize_essential_graph, step_global_bundle_adjustment, step_correct_se3]),
}
