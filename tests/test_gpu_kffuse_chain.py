"""-m gpu: one pass of the local-mapping thread over resident data, with the fuse in it: CreateNewMapPointsChain -> SearchInNeighborsFuse with
toy-map surgery -> RefreshMapPoints -> LocalBundleAdjustment.  Between the steps nothing is uploaded but flags, planes and what the surgery
changed.

The map is the chain scene of tests/_newpts_scenes.py (a current keyframe and three neighbours that see the same 40 world points) with an
OLD map laid under it: every neighbour feature that "already has a map point" holds a point of its own at the true position, so the same
world point lives in the store two or three times under different ids - the duplicates SearchInNeighbors exists to merge.  The fused map
must have the observation lists the sequential restatement (tests/_kffuse_ref.search_in_neighbors) gives on a host mirror of the store."""
import types

import numpy as np
import pytest

import _kffuse_ref as K
import _newpts_scenes as N
import _points_ref as R
import _tri_scenes as TS
from test_gpu_newpts_chain import CAPS, call_args, mask_dict
from test_gpu_triangulate import fill_slot

pytestmark = pytest.mark.gpu
KEY = (1, 3, 40, 32, 0)


def world_points(seed, n):
    """the first draws of _tri_scenes.World: the world points its features are projections of"""
    rng = np.random.default_rng(7000 + seed)
    return np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1, 1, n), rng.uniform(2.5, 8, n)], 1).astype(np.float32)


def host_mirror(store, cap, W, planes, grid):
    """the store and the slots as the restatement reads them"""
    every = np.arange(cap, dtype=np.int32)
    g = store.get(every)
    P = R.Points(cap)
    for a, b in (("pos", "pos"), ("normal", "normal"), ("min_distance", "min_distance"), ("max_distance", "max_distance"), ("ref_size", "ref_size"),
                 ("ref_distance", "ref_distance"), ("ref_sigma", "ref_sigma"), ("descriptors", "descriptors")):
        getattr(P, a)[:] = g[b]
    P.flags[:] = g["flags"]
    kfs = {}
    for s, kf in enumerate(W.kfs):
        c = W.cams[s]
        cam = R.Camera(Rcw=c["Rcw"], tcw=c["tcw"], Ow=c["Ow"], fx=c["fx"], fy=c["fy"], cx=c["cx"], cy=c["cy"], mbf=0.0)
        kfs[s] = K.Keyframe(kf.x, kf.y, kf.size, W.desc[s], planes[s].copy(), None, None, cam)
    return P, kfs


def test_fuse_between_new_points_and_local_bundle_adjustment(afv, gpu_ctx):
    ch = N.chain(*KEY)
    W, n, nn = ch.W, ch.n, ch.nn
    Pw = world_points(KEY[0], n)
    for s, kf in enumerate(W.kfs):        # the reconstruction is the scene's: every feature is its point's projection, a pixel of noise at most
        c = W.cams[s]
        pc = (c["Rcw"].reshape(3, 3) @ Pw.T).T + c["tcw"]
        assert np.all(np.abs(TS.FX * pc[:, 0] / pc[:, 2] + TS.CX - kf.x) < 2.0)
    cap, store_cap = CAPS[KEY], 512
    grid = K.Grid(0.0, 640.0, 0.0, 480.0, 64, 48)
    slots = list(range(nn + 1))
    table = afv.table.DescriptorTable(gpu_ctx, nn + 1, cap)
    store = afv.MapPoints(gpu_ctx, store_cap)
    try:
        table.set_camera(grid.min_x, grid.max_x, grid.min_y, grid.max_y, grid.cols, grid.rows, grid.inv_w, grid.inv_h)
        for s in slots:
            kf, c = W.kfs[s], W.cams[s]
            fill_slot(table, s, kf, W.desc[s], featvec=True)
            table.set_inf(s, np.float32(1.0) / (kf.size * kf.size))
            table.set_pose(s, c["Rcw"], c["tcw"], c["Ow"], c["fx"], c["fy"], c["cx"], c["cy"], 0.0)
        # the old map: a point of its own under every feature whose mask says "has a map point"
        masks = mask_dict(ch)
        planes = {s: np.full(n, -1, np.int32) for s in slots}
        obs_old = []
        for s in slots:
            for j in np.flatnonzero(masks[s]):
                pid = 100 + s * n + int(j)
                planes[s][j] = pid
                obs_old.append((pid, s, int(j)))
        old = np.array([o[0] for o in obs_old], np.int32)
        store.set(old, pos=np.stack([Pw[o[2]] for o in obs_old]))
        store.set_flags(old, bad=np.zeros(len(old)), observed=np.ones(len(old)))
        centres = {s: W.cams[s]["Ow"] for s in slots}
        max_size = {s: np.float32(TS.TOL) ** 7 for s in slots}
        st, _, _ = afv.RefreshMapPoints(table, store, slots, centres, max_size, old, {int(o[0]): o[1] for o in obs_old}, obs_old)
        assert not st.any()

        # 1. CreateNewMapPoints: the new points land in the store, the host learns their observations
        nbs, cams, F12, ep = call_args(ch)
        made = table.CreateNewMapPointsChain(store, 0, nbs, cams, F12, ep, ch.th_low, masks, ch.first_id)
        assert len(made) == 34
        new = np.array([pid for pid, _ in made], np.int32)
        for pid, two in made:
            for s, i in two:
                assert planes[s][i] == -1
                planes[s][i] = pid
        store.set_flags(new, bad=np.zeros(len(new)), observed=np.ones(len(new)))
        for s in slots:
            table.set_map_points(s, planes[s])

        # 2. SearchInNeighbors: the device answers target by target, the toy map does the surgery, flags and planes go back
        P_ref, kfs_ref = host_mirror(store, store_cap, W, planes, grid)
        M_ref = K.ToyMap(P_ref, kfs_ref)
        want = K.search_in_neighbors(M_ref, grid, 0, nbs, th_low=ch.th_low)
        P_dev = types.SimpleNamespace(flags=host_mirror(store, store_cap, W, planes, grid)[0].flags)
        kfs_dev = {s: types.SimpleNamespace(plane=planes[s], n=n) for s in slots}
        M_dev = K.ToyMap(P_dev, kfs_dev)
        known = np.concatenate([old, new])

        def on_fuse(s, ids, best, occupant, status):
            M_dev.apply(s, ids, best, status)
            store.set_flags(known, bad=(P_dev.flags[known] & R.BAD) != 0)
            for t in slots:
                table.set_map_points(t, planes[t])
        got = table.SearchInNeighborsFuse(store, 0, nbs, lambda: planes[0].copy(), lambda s: planes[s].copy(), on_fuse, th_low=ch.th_low)
        assert (got[0], got[1]) == want and sum(want[0]) + want[1] > 20
        assert M_dev.lists() == M_ref.lists()
        merged = [p for p in known if M_dev.is_bad(int(p))]
        assert len(merged) > 10                                   # duplicates went away ...
        lists = M_dev.lists()
        assert max(len(v) for v in lists.values()) >= 3           # ... and their observations went to the survivors
        for s in slots:
            assert np.array_equal(table.get_map_points(s, n), planes[s])
            assert len(set(planes[s][planes[s] >= 0].tolist())) == int((planes[s] >= 0).sum())   # a point sits on one feature of a keyframe

        # 3. the points of the current keyframe: ComputeDistinctiveDescriptors and UpdateNormalAndDepth (LocalMapping.cc:538-551)
        mine = sorted(set(int(p) for p in planes[0] if p >= 0))
        obs = [(p, s, i) for p in mine for s, i in lists[p]]
        ref_kf = {p: lists[p][0][0] for p in mine}
        st, best_obs, _ = afv.RefreshMapPoints(table, store, slots, centres, max_size, mine, ref_kf, obs)
        assert not st.any() and np.all(best_obs >= 0)

        # 4. LocalBundleAdjustment over what the fuse left: keyframe 1 plays keyId 0
        lba_cams = {s: dict(Rcw=W.cams[s]["Rcw"], tcw=W.cams[s]["tcw"], fx=TS.FX, fy=TS.FY, cx=TS.CX, cy=TS.CY, mbf=50.0) for s in slots}
        poses, xyz, erase, trace = afv.LocalBundleAdjustment(table, store, [(0, False), (1, True)], [2, 3], lba_cams, mine, obs)
        assert trace["n_edges"] == len(obs) and set(poses) == {0} and np.all(np.isfinite(xyz))
        moved = store.get(np.array(mine, np.int32))["pos"]
        assert np.allclose(moved, xyz.astype(np.float32)) and np.abs(moved - Pw[[lists[p][0][1] for p in mine]]).max() < 1.0
    finally:
        store.close()
        table.close()
