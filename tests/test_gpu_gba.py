"""-m gpu: afv_table_global_bundle_adjust (csrc/k_gba.hip: the block-sparse solve, deviation L7') and afv_points_correct_se3.

Every small scene of tests/_gba_scenes.py against the restatement tests/_gba_ref.py, and every scene of tests/_lba_scenes.py through the
NEW entry point against tests/_lba_ref.py, bit for bit: the pose and point doubles, the counts, the per-edge states and the trace.  Both
entry points on one input give the same bytes.  Past the old cap of 64 free keyframes the device is held against the host program
(tools/lba_host.cpp, gba_host; itself held to the restatement by tests/test_gba_host_cpu.py) on scenes sized by what the kernels stride
over.  write_points 0 / 1, two calls in a row, a cloned table, the refusals with outputs and store untouched (AFV_ECAPACITY included: one
point seen by 1448 keyframes fills more blocks than AFV_GBA_MAX_L_BLOCKS), a stop flag raised before the call, the trial budget, the
Python class; the float point correction against its restatement.  Nothing here provokes a fault: every input is finite and handled by
rule."""
import ctypes as C

import numpy as np
import pytest

import _gba_ref as G
import _gba_scenes as GS
import _lba_scenes as S
from test_gba_host_cpu import build_gba_host, expected, run_gba_host
from test_gpu_lba import Rig, assert_equal, want_ref

pytestmark = pytest.mark.gpu
SMALL = dict(GS.small())
OLD = dict(S.every_scene())
NEW, OLD_ENTRY = "afv_table_global_bundle_adjust", "afv_table_bundle_adjust"
_cache = {}


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return build_gba_host(tmp_path_factory.mktemp("gba_host_gpu") / "gba_host.so")


@pytest.fixture(scope="module")
def large_scenes():
    return GS.large()


class GRig(Rig):
    """Rig with the entry point as an argument"""

    def call(self, table=None, points=None, out=None, stop=None, prm="scene", entry=NEW, **over):
        sc = self.sc
        pad = lambda a: np.ascontiguousarray(a, np.int32) if len(a) else np.zeros(1, np.int32)
        a = dict(slots=pad(self.slots), nk=sc.nk, nf=sc.nf, cams=self.cams(), ids=pad(sc.ids), npts=sc.np, op=pad(sc.e_pt), ok=pad(sc.e_kf),
                 oi=pad(sc.e_idx), ne=sc.ne, prm=self.params() if isinstance(prm, str) else prm)
        a.update(over)
        res, kf, xyz, state = out or self.outputs()
        for k, v in (("res", res), ("kf", kf), ("xyz", xyz), ("state", state)):
            a.setdefault(k, v)
        p = lambda v: self.afv._lib.ptr(v) if isinstance(v, np.ndarray) else v
        code = getattr(self.table.lib, entry)((table or self.table).handle, (points or self.points).handle, p(a["slots"]), a["nk"], a["nf"], a["cams"],
                                              p(a["ids"]), a["npts"], p(a["op"]), p(a["ok"]), p(a["oi"]), a["ne"],
                                              None if a["prm"] is None else C.byref(a["prm"]), None if stop is None else C.byref(stop),
                                              None if a["res"] is None else C.byref(a["res"]), p(a["kf"]), p(a["xyz"]), p(a["state"]))
        return code, res, kf[:sc.nf], xyz[:sc.np], state[:sc.ne]


def want_sparse(name, sc, stop_at="scene"):
    def solve():
        r = sc.solve_sparse(stop_at=stop_at)
        return expected(r) + (np.concatenate([r.R, r.t], 1), r.xyz, r.state)
    return cached((name, stop_at), solve)


def run(afv, ctx, name, sc, want, **kw):
    rig = GRig(afv, ctx, sc)
    try:
        code, res, kf, xyz, state = rig.call(**kw)
        assert code == 0, (name, rig.table.lib.afv_last_error(ctx.handle))
        assert_equal((res, kf, xyz, state), want, name)
    finally:
        rig.close()


@pytest.mark.parametrize("name", sorted(SMALL))
def test_every_small_scene_against_the_sparse_restatement(afv, gpu_ctx, name):
    run(afv, gpu_ctx, name, SMALL[name], want_sparse(name, SMALL[name]))


@pytest.mark.parametrize("name", sorted(n for n in OLD if n != "stop_before"))
def test_every_scene_of_the_old_entry_point_through_the_new_one(afv, gpu_ctx, name):
    run(afv, gpu_ctx, name, OLD[name], want_ref(name, OLD[name]))


def test_stop_before_writes_nothing(afv, gpu_ctx):
    sc = OLD["stop_before"]
    rig = GRig(afv, gpu_ctx, sc)
    try:
        before = rig.points.get(sc.ids)
        code, res, kf, xyz, state = rig.call(out=rig.outputs(), stop=C.c_int32(1))
        assert code == 0 and res.stopped == 1 and not any(list(res.iterations) + list(res.trials) + [res.n_removed_first, res.n_erase])
        assert np.all(kf == 7.5) and np.all(xyz == 7.5) and np.all(state == 0xA5)
        assert rig.points.get(sc.ids)["pos"].tobytes() == before["pos"].tobytes()
        code, res, kf, xyz, state = rig.call(stop=C.c_int32(0))              # a flag that stays down changes nothing
        assert code == 0
        assert_equal((res, kf, xyz, state), want_ref("stop_before", sc, stop_at=None), "flag down")
    finally:
        rig.close()


@pytest.mark.parametrize("name", ["free_64", "arrow_fill", "pattern_empties"])
def test_both_entry_points_give_the_same_bytes(afv, gpu_ctx, name):
    sc = S.large_sized()["free_64"] if name == "free_64" else SMALL[name]
    rig = GRig(afv, gpu_ctx, sc)
    try:
        outs = []
        for entry in (OLD_ENTRY, NEW):
            code, res, kf, xyz, state = rig.call(entry=entry, prm=rig.params(write_points=0))
            assert code == 0, entry
            outs.append((bytes(res), kf.tobytes(), xyz.tobytes(), state.tobytes()))
        assert outs[0] == outs[1]
        assert res.iterations[0] >= 1 and res.n_edges == int(sc.p_ok[sc.e_pt].sum())
    finally:
        rig.close()


@pytest.mark.parametrize("name", ["band_65", "band_130", "hub_180", "band_65_checks"])
def test_past_the_old_cap_against_the_host_program(afv, gpu_ctx, host_lib, large_scenes, name):
    sc = GS.band_65_with_checks() if name == "band_65_checks" else large_scenes[name]
    want, extra, rc = run_gba_host(host_lib, sc)
    assert rc == 0 and extra[2] == 0 and want[0][0] >= 1
    rig = GRig(afv, gpu_ctx, sc)
    try:
        assert rig.call(entry=OLD_ENTRY)[0] == afv._lib.EINVAL               # the old entry point keeps its cap
        code, res, kf, xyz, state = rig.call()
        assert code == 0, rig.table.lib.afv_last_error(gpu_ctx.handle)
        assert_equal((res, kf, xyz, state), want, name)
    finally:
        rig.close()


def test_write_points_two_calls_in_a_row_and_a_cloned_table(afv, gpu_ctx):
    sc = SMALL["isolated_keyframe"]                                          # it has dropped points
    want = want_sparse("isolated_keyframe", sc)
    rig = GRig(afv, gpu_ctx, sc)
    dst = afv.table.DescriptorTable(gpu_ctx, sc.nk + 1, rig.cap)
    try:
        before = rig.points.get(sc.ids)
        code, res, kf, xyz, state = rig.call(prm=rig.params(write_points=0))
        assert code == 0
        assert_equal((res, kf, xyz, state), want, "write_points 0")
        after = rig.points.get(sc.ids)
        assert after["pos"].tobytes() == before["pos"].tobytes() and np.array_equal(after["flags"], before["flags"])   # the store stays
        rig.table.clone_into(dst)
        code, res, kf, xyz, state = rig.call(table=dst)
        assert code == 0
        assert_equal((res, kf, xyz, state), want, "write_points 1, cloned table")
        after = rig.points.get(sc.ids)
        ok = sc.p_ok.astype(bool)
        assert after["pos"][ok].tobytes() == xyz[ok].astype(np.float32).tobytes()        # the SetWorldPos cast
        assert after["pos"][~ok].tobytes() == before["pos"][~ok].tobytes() and np.all(xyz[~ok] == 0.0)
        again = S.Scene.__new__(S.Scene)                                                 # the second call starts from the first's positions
        again.__dict__.update(sc.__dict__)
        again.pos = np.where(ok[:, None], xyz.astype(np.float32), sc.pos)
        r = G.bundle_adjust(again.problem(), sc.iterations, sc.robust, sc.checks, sc.stop_at)
        code, res, kf, xyz, state = rig.call()
        assert code == 0
        assert_equal((res, kf, xyz, state), expected(r) + (np.concatenate([r.R, r.t], 1), r.xyz, r.state), "second call")
    finally:
        dst.close()
        rig.close()


@pytest.mark.parametrize("budget", [1, 2, 5])
def test_the_trial_budget(afv, gpu_ctx, budget):
    """band runs its first optimize() in 5 trials: inside it, and at its last trial (bDoMore = false)"""
    sc = SMALL["band"]
    full = want_sparse("band", sc)
    assert full[0][2] == 5
    rig = GRig(afv, gpu_ctx, sc)
    try:
        code, res, kf, xyz, state = rig.call(prm=rig.params(trial_budget=budget))
        assert code == 0 and res.stopped == 2
        assert_equal((res, kf, xyz, state), want_sparse("band", sc, stop_at=budget), budget)
    finally:
        rig.close()


def test_refusals_leave_outputs_and_store_untouched(afv, gpu_ctx):
    L = afv._lib
    sc = SMALL["mixed_mono_stereo"]
    rig = GRig(afv, gpu_ctx, sc)
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
        for f, v in (("checks", 2), ("write_points", -1), ("trial_budget", -1)):
            assert refused(prm=rig.params(**{f: v})) == L.EINVAL, f
        assert refused(nk=L.GBA_MAX_KF + 1) == L.EINVAL and refused(nf=sc.nk + 1) == L.EINVAL and refused(nf=-1) == L.EINVAL
        assert refused(npts=L.GBA_MAX_POINTS + 1) == L.EINVAL and refused(ne=L.GBA_MAX_EDGES + 1) == L.EINVAL and refused(ne=-1) == L.EINVAL
        assert refused(slots=changed(rig.slots, 1, sc.nk + 1)) == L.EINVAL
        assert refused(ids=changed(sc.ids, 3, sc.store_cap)) == L.EINVAL and refused(ids=changed(sc.ids, 3, sc.ids[4])) == L.EINVAL
        assert refused(op=changed(sc.e_pt, 9, 0)) == L.EINVAL           # not grouped by point
        assert refused(ok=changed(sc.e_kf, 9, sc.nk)) == L.EINVAL
        assert refused(ok=changed(sc.e_kf, 1, sc.e_kf[0])) == L.EINVAL  # a point observed twice by one keyframe
        assert refused(oi=changed(sc.e_idx, 9, -1)) == L.EINVAL
        assert b"afv_table_global_bundle_adjust" in rig.table.lib.afv_last_error(rig.ctx.handle)
        assert rig.points.get(sc.ids)["pos"].tobytes() == before
    finally:
        rig.close()


def test_a_fill_beyond_the_block_cap_answers_ecapacity(afv, gpu_ctx):
    """one point seen by 1448 free keyframes: every pair is structural, 1448 * 1449 / 2 = 1 049 076 blocks > AFV_GBA_MAX_L_BLOCKS.  Refused
    before any launch; with 1447 keyframes the plan fits, and the call would run"""
    L = afv._lib
    nf = 1448
    assert nf * (nf + 1) // 2 > L.GBA_MAX_L_BLOCKS >= (nf - 1) * nf // 2
    table = afv.table.DescriptorTable(gpu_ctx, 2, 4)
    points = afv.MapPoints(gpu_ctx, 8)
    try:
        table.set(1, np.zeros((1, 32), np.uint8))
        table.set_geometry(1, np.float32([320.0]), np.float32([240.0]), np.ones(1, np.float32), u_right=np.float32([-1.0]))
        table.set_inf(1, np.ones(1, np.float32))
        points.set(np.int32([3]), pos=np.float32([[0.0, 0.0, 5.0]]))
        before = points.get(np.int32([3]))["pos"].tobytes()
        # the refusal is taken on the edge list alone: every keyframe may name the same slot (the observations of one point by distinct
        # keyframes are distinct edges)
        slots = np.ones(nf, np.int32)
        cams = (L.LbaCam * nf)()
        for c in cams:
            c.struct_size = C.sizeof(L.LbaCam)
            c.Rcw[0] = c.Rcw[4] = c.Rcw[8] = 1.0
            c.fx, c.fy, c.cx, c.cy = 500.0, 500.0, 320.0, 240.0
        prm = L.sized(L.LbaParams)
        prm.iterations[0], prm.write_points = 10, 1
        res = L.LbaResult()
        C.memset(C.byref(res), 0xA5, C.sizeof(res))
        kf, xyz, state = np.full((nf, 12), 7.5), np.full((1, 3), 7.5), np.full(nf, 0xA5, np.uint8)
        ids, op, ok, oi = np.int32([3]), np.zeros(nf, np.int32), np.arange(nf, dtype=np.int32), np.zeros(nf, np.int32)
        p = L.ptr
        code = table.lib.afv_table_global_bundle_adjust(table.handle, points.handle, p(slots), nf, nf, cams, p(ids), 1, p(op), p(ok), p(oi), nf,
                                                        C.byref(prm), None, C.byref(res), p(kf), p(xyz), p(state))
        assert code == L.ECAPACITY and b"AFV_GBA_MAX_L_BLOCKS" in table.lib.afv_last_error(gpu_ctx.handle)
        assert bytes(res) == b"\xa5" * C.sizeof(res) and np.all(kf == 7.5) and np.all(xyz == 7.5) and np.all(state == 0xA5)
        assert points.get(np.int32([3]))["pos"].tobytes() == before
    finally:
        points.close()
        table.close()


def test_the_python_class(afv, gpu_ctx):
    sc = SMALL["arrow_fill"]
    rig = GRig(afv, gpu_ctx, sc)
    try:
        cams = {int(rig.slots[k]): dict(Rcw=sc.cams[k, :9], tcw=sc.cams[k, 9:12], fx=sc.cams[k, 12], fy=sc.cams[k, 13], cx=sc.cams[k, 14],
                                        cy=sc.cams[k, 15], mbf=sc.cams[k, 16]) for k in range(sc.nk)}
        obs = [(int(sc.ids[sc.e_pt[e]]), int(rig.slots[sc.e_kf[e]]), int(sc.e_idx[e])) for e in range(sc.ne)]
        r = cached("arrow_fill loop", lambda: G.bundle_adjust(sc.problem(), (10, 0), (False, False), False))
        before = rig.points.get(sc.ids)["pos"].tobytes()
        kfs = [(int(rig.slots[k]), k >= sc.nf) for k in range(sc.nk)]
        poses, xyz, trace = afv.GlobalBundleAdjustment(rig.table, rig.points, kfs, cams, sc.ids, obs, 10, robust=False, write_points=False)
        assert xyz.tobytes() == r.xyz.tobytes() and trace["iterations"] == [int(r.iterations[0]), 0] and trace["trials"][0] == r.trials[0]
        for i in range(sc.nf):
            Rk, tk = poses[int(rig.slots[i])]
            assert np.concatenate([Rk.reshape(9), tk]).tobytes() == np.concatenate([r.R[i], r.t[i]]).tobytes()
        assert rig.points.get(sc.ids)["pos"].tobytes() == before                          # PosGBA stays with the caller
    finally:
        rig.close()


def seeded_transforms(m, seed):
    rng = np.random.default_rng(seed)
    T = np.zeros((2, m, 12), np.float32)
    for s in range(2):
        for q in range(m):
            a, ax = rng.uniform(-1, 1), rng.normal(0, 1, 3)
            ax /= np.linalg.norm(ax)
            K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
            T[s, q, :9] = (np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K).reshape(9)
            T[s, q, 9:] = rng.uniform(-3, 3, 3)
    return T


@pytest.mark.parametrize("n,m", [(1, 1), (63, 7), (64, 1), (65, 7), (300, 7)])
def test_correct_se3_against_the_restatement(afv, gpu_ctx, n, m):
    L = afv._lib
    rng = np.random.default_rng(100 + n)
    T = seeded_transforms(m, n)
    cap = 2 * n + 9
    points = afv.MapPoints(gpu_ctx, cap)
    try:
        ids = rng.permutation(cap)[:n].astype(np.int32)
        pos = rng.uniform(-8, 8, (n, 3)).astype(np.float32)
        is_set = np.ones(n, bool)
        bad = np.zeros(n, bool)
        pair = rng.integers(0, m, n).astype(np.int32)
        if n >= 63:
            is_set[[5, 40]] = False
            bad[[7, 62]] = True
            pair[[3, 7, 50]] = -1
        points.set(ids[is_set], pos=pos[is_set])
        points.set_flags(ids[is_set], bad=bad[is_set].astype(np.float32), observed=np.ones(int(is_set.sum())))
        before = points.get(ids)["pos"].copy()
        want, want_st = G.correct_se3(before, is_set & ~bad, pair, T[0], T[1])
        st = points.correct_se3(ids, pair, T[0], T[1])
        assert np.array_equal(st, want_st) and (n < 63 or set(st) == {L.POINT_MOVED, L.POINT_BAD_OR_UNSET, L.POINT_NO_PAIR})
        got = points.get(ids)["pos"]
        assert got.tobytes() == want.tobytes()
        assert got[st == L.POINT_MOVED].tobytes() != before[st == L.POINT_MOVED].tobytes()
        # refusals: the store stays
        assert points.lib.afv_points_correct_se3(points.handle, L.ptr(ids), n, L.ptr(np.full(n, m, np.int32)), L.ptr(T[0]), L.ptr(T[1]), m,
                                                 L.ptr(np.zeros(n, np.uint8))) == L.EINVAL
        nan = T[0].copy()
        nan[0, 4] = np.nan
        assert points.lib.afv_points_correct_se3(points.handle, L.ptr(ids), n, L.ptr(pair), L.ptr(nan), L.ptr(T[1]), m,
                                                 L.ptr(np.zeros(n, np.uint8))) == L.EINVAL
        assert points.get(ids)["pos"].tobytes() == got.tobytes()
    finally:
        points.close()
