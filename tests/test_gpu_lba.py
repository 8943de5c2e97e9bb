"""-m gpu: afv_table_bundle_adjust (csrc/k_lba.hip) against the restatement (tests/_lba_ref.py) on every constructed scene and against the
host program (tools/lba_host.cpp, itself held to the restatement by tests/test_lba_host_cpu.py) on the sized scenes, bit for bit: the pose
and point doubles, the counts, the per-edge states and the trace of both optimize() calls.  The three table kinds; a cloned table and a
slot promoted from a frame (both must bring the planes); write_points 0 / 1 read back through afv_points_get; dropped points; the trial
budget at each place the restatement distinguishes; a stop flag raised before the call; two calls in a row; every refusal with the
outputs untouched; the Python classes; the chain create_new_points -> LocalBundleAdjustment -> SearchLocalPoints.  Nothing here provokes a fault: every input is finite and handled by rule."""
import ctypes as C

import numpy as np
import pytest

import _lba_ref as R
import _lba_scenes as S
from test_lba_host_cpu import build_host, expected, run_host

pytestmark = pytest.mark.gpu
SCENES = dict(S.every_scene())
_cache = {}


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("lba_host_gpu") / "lba_host.so")


class Rig:
    """a scene installed in a table (keyframe k: slot nk - k, slot 0 stays empty) and a store (point p: id sc.ids[p])"""

    def __init__(self, afv, ctx, sc, desc_bytes=32, float_dim=0, skip=()):
        self.afv, self.ctx, self.sc = afv, ctx, sc
        kind = {"float_dim": float_dim} if float_dim else {"desc_bytes": desc_bytes}
        self.cap = max([len(f["x"]) for f in sc.feats] + [1]) + 2
        self.table = afv.table.DescriptorTable(ctx, sc.nk + 1, self.cap, **kind)
        self.points = afv.MapPoints(ctx, sc.store_cap, **kind)
        self.slots = np.array([sc.nk - k for k in range(sc.nk)], np.int32)
        rng = np.random.default_rng(4)
        for k, f in enumerate(sc.feats):
            if k in skip:
                continue
            n = len(f["x"])
            rows = rng.normal(0, 1, (n, float_dim)).astype(np.float32) if float_dim else rng.integers(0, 256, (n, desc_bytes), dtype=np.uint8)
            self.table.set(int(self.slots[k]), rows)
            self.table.set_geometry(int(self.slots[k]), f["x"], f["y"], np.ones(n, np.float32), u_right=f["ur"])
            self.table.set_inf(int(self.slots[k]), f["inf"])
        ok = np.nonzero(sc.p_ok)[0]
        if len(ok):
            self.points.set(sc.ids[ok], pos=sc.pos[ok])

    def close(self):
        self.points.close()
        self.table.close()

    def cams(self):
        L = self.afv._lib
        cams = (L.LbaCam * max(self.sc.nk, 1))()
        for k in range(self.sc.nk):
            c = cams[k]
            c.struct_size = C.sizeof(L.LbaCam)
            for q in range(9):
                c.Rcw[q] = float(self.sc.cams[k, q])
            for q in range(3):
                c.tcw[q] = float(self.sc.cams[k, 9 + q])
            c.fx, c.fy, c.cx, c.cy, c.bf = (float(v) for v in self.sc.cams[k, 12:17])
        return cams

    def params(self, **over):
        L, sc = self.afv._lib, self.sc
        p = L.sized(L.LbaParams)
        p.iterations[0], p.iterations[1], p.robust[0], p.robust[1] = sc.iterations[0], sc.iterations[1], int(sc.robust[0]), int(sc.robust[1])
        p.checks, p.write_points, p.trial_budget = int(sc.checks), 1, 0 if not sc.stop_at else sc.stop_at
        for k, v in over.items():
            setattr(p, k, v)
        return p

    def outputs(self, poison=0xA5):
        L, sc = self.afv._lib, self.sc
        res = L.LbaResult()
        C.memset(C.byref(res), poison, C.sizeof(res))
        return res, np.full((max(sc.nf, 1), 12), 7.5), np.full((max(sc.np, 1), 3), 7.5), np.full(max(sc.ne, 1), poison, np.uint8)

    def call(self, table=None, points=None, out=None, stop=None, prm="scene", **over):
        """the C entry point as it is: returns (code, result, kf, xyz, state).  Outputs start poisoned: what the call leaves is what it wrote"""
        sc = self.sc
        pad = lambda a: np.ascontiguousarray(a, np.int32) if len(a) else np.zeros(1, np.int32)
        a = dict(slots=pad(self.slots), nk=sc.nk, nf=sc.nf, cams=self.cams(), ids=pad(sc.ids), npts=sc.np, op=pad(sc.e_pt), ok=pad(sc.e_kf),
                 oi=pad(sc.e_idx), ne=sc.ne, prm=self.params() if isinstance(prm, str) else prm)
        a.update(over)
        res, kf, xyz, state = out or self.outputs()
        for k, v in (("res", res), ("kf", kf), ("xyz", xyz), ("state", state)):
            a.setdefault(k, v)
        p = lambda v: self.afv._lib.ptr(v) if isinstance(v, np.ndarray) else v
        code = self.table.lib.afv_table_bundle_adjust((table or self.table).handle, (points or self.points).handle, p(a["slots"]), a["nk"], a["nf"],
                                                      a["cams"], p(a["ids"]), a["npts"], p(a["op"]), p(a["ok"]), p(a["oi"]), a["ne"],
                                                      None if a["prm"] is None else C.byref(a["prm"]), None if stop is None else C.byref(stop),
                                                      None if a["res"] is None else C.byref(a["res"]), p(a["kf"]), p(a["xyz"]), p(a["state"]))
        return code, res, kf[:sc.nf], xyz[:sc.np], state[:sc.ne]


def got_ints(g):
    return np.array(list(g.iterations) + list(g.trials) + [g.n_edges, g.n_removed_first, g.n_erase, g.stopped], np.int32)


def assert_equal(out, want, name):
    """(result, kf, xyz, state) of a call against (ints[8], doubles[4], kf, xyz, state), bit for bit"""
    g, kf, xyz, state = out
    assert np.array_equal(got_ints(g), want[0]), (name, got_ints(g), want[0])
    got = np.array(list(g.chi2) + list(g.lam), np.float64)
    assert got.tobytes() == want[1].tobytes(), (name, got, want[1])
    assert kf.tobytes() == want[2].tobytes(), name
    assert xyz.tobytes() == want[3].tobytes(), name
    assert np.array_equal(state, want[4]), name


def want_ref(name, sc, stop_at="scene"):
    def solve():
        r = sc.solve(stop_at=stop_at)
        ints, doubles = expected(r)
        return ints, doubles, np.concatenate([r.R, r.t], 1), r.xyz, r.state
    return cached((name, stop_at), solve)


def run(afv, ctx, name, sc, want, **kind):
    rig = Rig(afv, ctx, sc, **kind)
    try:
        code, res, kf, xyz, state = rig.call()
        assert code == 0, (name, rig.table.lib.afv_last_error(ctx.handle))
        assert_equal((res, kf, xyz, state), want, name)
        return rig, res
    finally:
        rig.close()


@pytest.mark.parametrize("name", sorted(n for n in SCENES if n != "stop_before"))
def test_every_constructed_scene_against_the_restatement(afv, gpu_ctx, name):
    sc = SCENES[name]
    run(afv, gpu_ctx, name, sc, want_ref(name, sc))


@pytest.mark.parametrize("name", sorted(S.small_sized()) + sorted(S.large_sized()))
def test_sized_scenes_against_the_host_program(afv, gpu_ctx, host_program, name):
    sc = dict(S.small_sized(), **S.large_sized())[name]
    run(afv, gpu_ctx, name, sc, run_host(host_program, sc))


@pytest.mark.parametrize("kind", [dict(desc_bytes=32), dict(desc_bytes=61), dict(float_dim=128)])
def test_table_and_store_kinds_give_the_same_answer(afv, gpu_ctx, kind):
    run(afv, gpu_ctx, "mixed_mono_stereo", SCENES["mixed_mono_stereo"], want_ref("mixed_mono_stereo", SCENES["mixed_mono_stereo"]), **kind)


def test_a_cloned_table_brings_the_planes(afv, gpu_ctx):
    sc = SCENES["mixed_mono_stereo"]
    rig = Rig(afv, gpu_ctx, sc)
    dst = afv.table.DescriptorTable(gpu_ctx, sc.nk + 1, rig.cap)
    try:
        rig.table.clone_into(dst)
        code, res, kf, xyz, state = rig.call(table=dst)
        assert code == 0
        assert_equal((res, kf, xyz, state), want_ref("mixed_mono_stereo", sc), "clone")
    finally:
        dst.close()
        rig.close()


def test_a_slot_promoted_from_a_frame_brings_its_planes(afv, gpu_ctx):
    """keyframe 2 arrives through afv_table_set_from_frame: geometry, u_right (-1: a monocular frame) and keyPtsInf = 1 / size^2"""
    sc = S.make(seed=42, outliers=[(5, 2, 30.0)])
    f = sc.feats[2]
    n = len(f["x"])
    assert 10 < f["x"].min() and f["x"].max() < 630 and 10 < f["y"].min() and f["y"].max() < 470
    size = (np.float32(1.2) ** np.random.default_rng(1).integers(0, 4, n)).astype(np.float32)
    f["inf"] = (np.float32(1.0) / (size * size)).astype(np.float32)
    sc.obs[sc.e_kf == 2, 3] = f["inf"][sc.e_idx[sc.e_kf == 2]]
    rig = Rig(afv, gpu_ctx, sc, skip=(2,))
    fr = afv.Frame(gpu_ctx, max_x=640.0, max_y=480.0, cap=rig.cap)
    try:
        rig.table.set(int(rig.slots[2]), np.zeros((n, 32), np.uint8))
        assert rig.call()[0] == afv._lib.EINVAL                          # the slot holds features without geometry
        kps = np.zeros(n, afv.KP_DTYPE)
        kps["x"], kps["y"] = f["x"], f["y"]
        fr.set_features(kps, np.random.default_rng(2).integers(0, 256, (n, 32), dtype=np.uint8), sizes=size)
        rig.table.set_from_frame(int(rig.slots[2]), fr)
        code, res, kf, xyz, state = rig.call()
        assert code == 0
        r = sc.solve()
        assert_equal((res, kf, xyz, state), expected(r) + (np.concatenate([r.R, r.t], 1), r.xyz, r.state), "from frame")
    finally:
        fr.close()
        rig.close()


def test_write_points_dropped_points_and_two_calls_in_a_row(afv, gpu_ctx):
    sc = SCENES["dropped_points"]
    want = want_ref("dropped_points", sc)
    rig = Rig(afv, gpu_ctx, sc)
    try:
        before = rig.points.get(sc.ids)
        code, res, kf, xyz, state = rig.call(prm=rig.params(write_points=0))
        assert code == 0
        assert_equal((res, kf, xyz, state), want, "write_points 0")
        after = rig.points.get(sc.ids)
        assert after["pos"].tobytes() == before["pos"].tobytes() and np.array_equal(after["flags"], before["flags"])   # the store stays
        code, res, kf, xyz, state = rig.call()
        assert code == 0
        assert_equal((res, kf, xyz, state), want, "write_points 1")
        after = rig.points.get(sc.ids)
        ok = sc.p_ok.astype(bool)
        assert after["pos"][ok].tobytes() == xyz[ok].astype(np.float32).tobytes()        # the SetWorldPos cast
        assert after["pos"][~ok].tobytes() == before["pos"][~ok].tobytes() and np.all(xyz[~ok] == 0.0) and np.all(state[~ok[sc.e_pt]] == 0)
        # the second call starts from the first's written positions
        again = S.Scene.__new__(S.Scene)
        again.__dict__.update(sc.__dict__)
        again.pos = np.where(ok[:, None], xyz.astype(np.float32), sc.pos)
        r = again.solve()
        code, res, kf, xyz, state = rig.call()
        assert code == 0
        assert_equal((res, kf, xyz, state), expected(r) + (np.concatenate([r.R, r.t], 1), r.xyz, r.state), "second call")
    finally:
        rig.close()


@pytest.mark.parametrize("budget", [1, 2, 5, 6, 7, 14, 15, 16])
def test_the_trial_budget_at_each_place_the_restatement_distinguishes(afv, gpu_ctx, budget):
    """scene chi2_first_mono runs 5 + 10 trials: inside the first optimize(), at its last trial (bDoMore = false), inside the second, at
    its last trial, and beyond"""
    sc = SCENES["chi2_first_mono"]
    rig = Rig(afv, gpu_ctx, sc)
    try:
        code, res, kf, xyz, state = rig.call(prm=rig.params(trial_budget=budget))
        assert code == 0
        assert_equal((res, kf, xyz, state), want_ref("chi2_first_mono", sc, stop_at=budget), budget)
        assert res.stopped == (2 if budget <= 5 else 3 if budget <= 15 else 0)
    finally:
        rig.close()


def test_a_stop_flag_raised_before_the_call_writes_nothing(afv, gpu_ctx):
    sc = SCENES["stop_before"]
    rig = Rig(afv, gpu_ctx, sc)
    try:
        before = rig.points.get(sc.ids)
        out = rig.outputs()
        code, res, kf, xyz, state = rig.call(out=out, stop=C.c_int32(1))
        assert code == 0 and res.stopped == 1 and not any(list(res.iterations) + list(res.trials) + [res.n_removed_first, res.n_erase])
        assert np.all(kf == 7.5) and np.all(xyz == 7.5) and np.all(state == 0xA5)
        assert rig.points.get(sc.ids)["pos"].tobytes() == before["pos"].tobytes()
        code, res, kf, xyz, state = rig.call(stop=C.c_int32(0))              # a flag that stays down changes nothing
        assert code == 0
        assert_equal((res, kf, xyz, state), want_ref("stop_before", sc, stop_at=None), "flag down")
    finally:
        rig.close()


def test_refusals_leave_the_outputs_untouched(afv, gpu_ctx):
    L = afv._lib
    sc = SCENES["mixed_mono_stereo"]
    rig = Rig(afv, gpu_ctx, sc)
    other_ctx = afv.Context(max_width=640, max_height=480, max_batch=1)
    foreign = afv.MapPoints(other_ctx, 16)
    try:
        before = rig.points.get(sc.ids)["pos"].tobytes()

        def refused(**over):
            out = rig.outputs()
            code = rig.call(out=out, **over)[0]
            assert bytes(out[0]) == b"\xa5" * C.sizeof(out[0]) and np.all(out[1] == 7.5) and np.all(out[2] == 7.5) and np.all(out[3] == 0xA5), over.keys()
            return code

        def changed(a, i, v):
            b = np.array(a, np.int32)
            b[i] = v
            return b
        for k in ("slots", "cams", "ids", "op", "ok", "oi", "prm", "res", "kf", "xyz", "state"):
            assert refused(**{k: None}) == L.EINVAL, k
        bad = rig.params()
        bad.struct_size = 12
        assert refused(prm=bad) == L.EINVAL
        cams = rig.cams()
        cams[1].struct_size = 4
        assert refused(cams=cams) == L.EINVAL
        for f, v in (("checks", 2), ("write_points", -1), ("trial_budget", -1)):
            assert refused(prm=rig.params(**{f: v})) == L.EINVAL, f
        bad = rig.params()
        bad.iterations[1] = -1
        assert refused(prm=bad) == L.EINVAL
        bad = rig.params()
        bad.robust[0] = 2
        assert refused(prm=bad) == L.EINVAL
        assert refused(nk=L.LBA_MAX_KF + 1) == L.EINVAL and refused(nf=sc.nk + 1) == L.EINVAL and refused(nf=-1) == L.EINVAL
        assert refused(npts=L.LBA_MAX_POINTS + 1) == L.EINVAL and refused(ne=L.LBA_MAX_EDGES + 1) == L.EINVAL and refused(ne=-1) == L.EINVAL
        assert refused(slots=changed(rig.slots, 1, sc.nk + 1)) == L.EINVAL and refused(slots=changed(rig.slots, 0, -1)) == L.EINVAL
        assert refused(points=foreign) == L.EINVAL                      # a store of another context
        assert refused(ids=changed(sc.ids, 3, sc.store_cap)) == L.EINVAL and refused(ids=changed(sc.ids, 3, -1)) == L.EINVAL
        assert refused(ids=changed(sc.ids, 3, sc.ids[4])) == L.EINVAL   # named twice
        assert refused(op=changed(sc.e_pt, 9, sc.np)) == L.EINVAL and refused(op=changed(sc.e_pt, 9, -1)) == L.EINVAL
        assert refused(op=changed(sc.e_pt, 9, 0)) == L.EINVAL           # not grouped by point
        assert refused(ok=changed(sc.e_kf, 9, sc.nk)) == L.EINVAL and refused(ok=changed(sc.e_kf, 9, -1)) == L.EINVAL
        assert refused(ok=changed(sc.e_kf, 1, sc.e_kf[0])) == L.EINVAL  # a point observed twice by one keyframe
        n0 = len(sc.feats[sc.e_kf[9]]["x"])
        assert refused(oi=changed(sc.e_idx, 9, n0)) == L.EINVAL and refused(oi=changed(sc.e_idx, 9, -1)) == L.EINVAL
        f = sc.feats[1]
        rig.table.set(int(rig.slots[1]), np.zeros((len(f["x"]), 32), np.uint8))  # a recycled slot: without geometry, then without information
        assert refused() == L.EINVAL
        rig.table.set_geometry(int(rig.slots[1]), f["x"], f["y"], np.ones(len(f["x"])), u_right=f["ur"])
        assert refused() == L.EINVAL
        assert b"information" in rig.table.lib.afv_last_error(rig.ctx.handle)
        rig.table.set_inf(int(rig.slots[1]), f["inf"])
        assert rig.points.get(sc.ids)["pos"].tobytes() == before
        code, res, kf, xyz, state = rig.call()                            # ... and the call works again
        assert code == 0
        assert_equal((res, kf, xyz, state), want_ref("mixed_mono_stereo", sc), "after the refusals")
    finally:
        foreign.close()
        other_ctx.close()
        rig.close()


def test_the_python_classes(afv, gpu_ctx):
    """LocalBundleAdjustment / BundleAdjustment build the edge arrays from an observation list and order the keyframes free first"""
    sc = SCENES["mixed_mono_stereo"]
    rig = Rig(afv, gpu_ctx, sc)
    try:
        cams = {int(rig.slots[k]): dict(Rcw=sc.cams[k, :9], tcw=sc.cams[k, 9:12], fx=sc.cams[k, 12], fy=sc.cams[k, 13], cx=sc.cams[k, 14],
                                        cy=sc.cams[k, 15], mbf=sc.cams[k, 16]) for k in range(sc.nk)}
        obs = [(int(sc.ids[sc.e_pt[e]]), int(rig.slots[sc.e_kf[e]]), int(sc.e_idx[e])) for e in range(sc.ne)]
        want = want_ref("mixed_mono_stereo", sc)
        poses, xyz, erase, trace = afv.LocalBundleAdjustment(rig.table, rig.points, [int(s) for s in rig.slots[:sc.nf]],
                                                             [int(s) for s in rig.slots[sc.nf:]], cams, sc.ids, obs)
        assert xyz.tobytes() == want[3].tobytes() and np.array_equal(trace["edge_state"], want[4])
        for i in range(sc.nf):
            Rk, tk = poses[int(rig.slots[i])]
            assert np.concatenate([Rk.reshape(9), tk]).tobytes() == want[2][i].tobytes()
        assert erase == [(obs[e][1], obs[e][0]) for e in np.nonzero(want[4] == R.ERASE)[0]] and len(erase) == want[0][6]
        assert trace["iterations"] == list(want[0][:2]) and trace["trials"] == list(want[0][2:4])
    finally:
        rig.close()
    sc = SCENES["startup_two_keyframes"]
    rig = Rig(afv, gpu_ctx, sc)
    try:
        cams = {int(rig.slots[k]): dict(Rcw=sc.cams[k, :9], tcw=sc.cams[k, 9:12], fx=sc.cams[k, 12], fy=sc.cams[k, 13], cx=sc.cams[k, 14],
                                        cy=sc.cams[k, 15], mbf=sc.cams[k, 16]) for k in range(sc.nk)}
        obs = [(int(sc.ids[sc.e_pt[e]]), int(rig.slots[sc.e_kf[e]]), int(sc.e_idx[e])) for e in range(sc.ne)]
        want = want_ref("startup_two_keyframes", sc)
        # keyId == 0 comes first in the caller's list and is flagged fixed
        poses, xyz, trace = afv.BundleAdjustment(rig.table, rig.points, [(int(rig.slots[1]), True), (int(rig.slots[0]), False)], cams, sc.ids, obs,
                                                 nIterations=20, robust=False)
        assert xyz.tobytes() == want[3].tobytes() and list(poses) == [int(rig.slots[0])] and trace["iterations"][0] == 20
    finally:
        rig.close()


def test_the_chain_new_points_local_ba_search_local_points(afv, gpu_ctx):
    """create_new_points -> LocalBundleAdjustment -> SearchLocalPoints on one small map, nothing downloaded in between: the adjustment
    reads the points the chain just wrote and equals the restatement over them; the search then sees the moved points exactly as it sees a
    store that the host filled with the adjusted positions"""
    import _newpts_scenes as N
    from test_gpu_newpts_chain import CAPS, build_table, call_args, mask_dict
    from test_gpu_triangulate import FIELDS, prefilled_store
    key = (1, 3, 40, 32, 0)
    ch = N.chain(*key)
    W, want = ch.W, ch.want
    nbs, cams, F12, ep = call_args(ch)
    made, _ = prefilled_store(afv, gpu_ctx, 200)
    host, _ = prefilled_store(afv, gpu_ctx, 200)
    fr = afv.Frame(gpu_ctx, max_x=640.0, max_y=480.0, cap=320)
    t = None
    try:
        t = build_table(afv, gpu_ctx, ch, CAPS[key])
        got = t.CreateNewMapPointsChain(made, 0, nbs, cams, F12, ep, ch.th_low, mask_dict(ch), ch.first_id)
        ids = np.array([nid for nid, _ in got], np.int32)
        assert len(ids) == 34
        inf = [(np.float32(1.0) / np.asarray(W.kfs[k].sigma2, np.float32)).astype(np.float32) for k in range(ch.nn + 1)]
        for k in range(ch.nn + 1):
            t.set_inf(k, inf[k])
        obs = [(int(nid), int(slot), int(i)) for nid, pairs in got for slot, i in pairs]
        start = made.get(ids)["pos"].copy()
        # the current keyframe is optimised, its neighbours are fixed
        poses, xyz, erase, trace = afv.LocalBundleAdjustment(t, made, [0], list(range(1, ch.nn + 1)), cams, ids, obs)
        # ... the same problem through the restatement
        rec = np.zeros((ch.nn + 1, 17), np.float32)
        for k in range(ch.nn + 1):
            c = cams[k]
            rec[k, :9], rec[k, 9:12] = np.asarray(c["Rcw"], np.float32).reshape(9), np.asarray(c["tcw"], np.float32).reshape(3)
            rec[k, 12:17] = [c["fx"], c["fy"], c["cx"], c["cy"], c.get("mbf", c.get("bf", 0.0))]
        where = {int(p): i for i, p in enumerate(ids)}
        ur = [np.full(W.kfs[k].n, -1.0, np.float32) if W.kfs[k].u_right is None else np.asarray(W.kfs[k].u_right, np.float32) for k in range(ch.nn + 1)]
        e = np.array([(where[p], s, i) for p, s, i in obs], np.int32)
        rows = np.array([(W.kfs[s].x[i], W.kfs[s].y[i], ur[s][i], inf[s][i]) for _, s, i in obs], np.float32)
        r = R.bundle_adjust(R.Problem(rec, 1, start, np.ones(len(ids), np.uint8), e[:, 0], e[:, 1], rows))
        assert xyz.tobytes() == r.xyz.tobytes() and np.array_equal(trace["edge_state"], r.state)
        assert np.concatenate([poses[0][0].reshape(9), poses[0][1]]).tobytes() == np.concatenate([r.R[0], r.t[0]]).tobytes()
        assert trace["iterations"][0] > 0 and trace["n_edges"] == 2 * len(ids)
        moved = made.get(ids)["pos"]
        assert moved.tobytes() == xyz.astype(np.float32).tobytes() and moved.tobytes() != start.tobytes()
        # SearchLocalPoints: the store the chain and the adjustment wrote, against one filled by the host
        f = [w[4] for w in want]
        host.set(ids, **{k: np.stack([x[k] for x in f]) for k in FIELDS})
        host.set(ids, pos=moved)
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
