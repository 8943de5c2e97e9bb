"""-m gpu: afv_essential_graph and afv_points_correct_sim3 (csrc/k_essgraph.hip) against the restatement (tests/_essgraph_ref.py) on every
constructed scene and against the host program (tools/essgraph_host.cpp, itself held to the restatement by
tests/test_essgraph_host_cpu.py) on the sized scenes, bit for bit: S_out, Tiw_out, xyz_out, the statuses and the trace.  The sizes are the
edges of the kernel's shape: 2 and 3 keyframes; chains whose columns hold 1, 2, 16, 17 and 18 sub-diagonal blocks (16 wavefronts walk the
update triples, 1024 lanes the rows); chains of 65 and 130 with a loop edge from the last to the first free keyframe (arrow fill in every column);
vertices with 63, 64 and 65 edges (the 64-partial tree); fix_scale on and off; the floating component; a fill beyond
AFV_ESS_MAX_L_BLOCKS.  The point correction through both entries with 0, 1, 63, 64, 65 and 257 points, bad and unset points and points
without a reference, write_points 0, binary and float stores.  Two calls in a row; every refusal with the outputs and the store untouched;
the Python layer.  Nothing here provokes a fault: every input is finite and handled by rule."""
import ctypes as C

import numpy as np
import pytest

import _essgraph_host as H
import _essgraph_ref as G
import _essgraph_scenes as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return H.build_host(tmp_path_factory.mktemp("essgraph_host_gpu") / "essgraph_host.so")


def hubs():
    """vertex 0 fixed; hubs 1, 2, 3 with 63, 64 and 65 edges: one onto the fixed vertex, the others from leaves 4 .."""
    n = 4 + 64
    truth = SC.circle(n, 1.05)
    init = [(SC.rot([0.01 * (k % 7), 0, 0.002 * k]) @ R, t, 1.0) if k else (R, t, s) for k, (R, t, s) in enumerate(truth)]
    edges = [(1, 0), (2, 0), (3, 0)]
    for leaf in range(64):
        edges += [(4 + leaf, h) for h, cnt in ((1, 62), (2, 63), (3, 64)) if leaf < cnt]
    return SC.scene(init, 0, edges, truth, iterations=3)


def loop_chain(n, band, **kw):
    """the loop edge joins the last keyframe with the first FREE one: eliminating that one first fills the last block row in every column"""
    return SC.drifted(n, band, edges=[(n - 1, 1)] + SC.band_edges(n, band, loop=False), **kw)


SIZED = {
    "two_keyframes": lambda: SC.drifted(2, 0, iterations=4),
    "chain_of_3": lambda: SC.drifted(3, 0, iterations=4),
    "band_0": lambda: SC.drifted(30, 0, iterations=3),
    "band_1": lambda: SC.drifted(30, 1, iterations=3),
    "band_15": lambda: SC.drifted(40, 15, iterations=3),
    "band_16": lambda: SC.drifted(40, 16, iterations=3),
    "band_17": lambda: SC.drifted(40, 17, iterations=3),
    "chain_65_loop": lambda: loop_chain(65, 0, iterations=3),
    "chain_130_loop": lambda: loop_chain(130, 0, iterations=3),
    "chain_130_fix_scale": lambda: loop_chain(130, 1, fix_scale=True, iterations=3),
    "chain_64_fixed_last": lambda: SC.drifted(64, 2, fixed=63, iterations=3),
    "hubs_63_64_65": hubs,
    "floating_sized": lambda: dict(SC.floating(), iterations=4),
}


def poisoned(nk, npts):
    return np.full((nk, 13), 7.5), np.full((nk, 12), 7.5), np.full((max(npts, 1), 3), 7.5), np.full(max(npts, 1), 0xA5, np.uint8)


def call(afv, ctx, sc, points=None, ids=None, ref=None, out=None, write_points=1, prm="scene", **over):
    """the C entry point as it is: (code, result, S_out, Tiw, xyz, status).  Outputs start poisoned: what the call leaves is what it wrote"""
    L = afv._lib
    S, M = H.records(sc["S_init"]), H.records(sc["meas"])
    nk, ne = len(S), len(sc["v0"])
    pad = lambda a, dt: np.ascontiguousarray(a, dt) if len(a) else np.zeros(16, dt)
    npts = 0 if ids is None else len(ids)
    if isinstance(prm, str):
        prm = L.sized(L.EssParams)
        prm.iterations, prm.lambda_init, prm.fix_scale, prm.write_points = sc["iterations"], 1e-16, int(sc["fix_scale"]), write_points
    res = L.EssResult()
    C.memset(C.byref(res), 0xA5, C.sizeof(res))
    S_out, Tiw, xyz, st = out or poisoned(nk, npts)
    a = dict(points=None if points is None else points.handle, S=S, nk=nk, fixed=sc["fixed"], v0=pad(sc["v0"], np.int32), v1=pad(sc["v1"], np.int32),
             M=pad(M, np.float64), ne=ne, prm=prm, ids=pad(ids if npts else [], np.int32), ref=pad(ref if npts else [], np.int32), npts=npts, res=res,
             S_out=S_out, Tiw=Tiw, xyz=xyz, st=st)
    a.update(over)
    for k in ("points", "ids", "ref"):                       # a refusal case replaces one of these behind the helper's back
        if k + "_raw" in a:
            a[k] = a[k + "_raw"]
    p = lambda v: L.ptr(v) if isinstance(v, np.ndarray) else v
    code = ctx.lib.afv_essential_graph(ctx.handle, a["points"], p(a["S"]), a["nk"], a["fixed"], p(a["v0"]), p(a["v1"]), p(a["M"]), a["ne"],
                                       None if a["prm"] is None else C.byref(a["prm"]), p(a["ids"]), p(a["ref"]), a["npts"],
                                       None if a["res"] is None else C.byref(a["res"]), p(a["S_out"]), p(a["Tiw"]), p(a["xyz"]), p(a["st"]))
    return code, res, S_out, Tiw, xyz[:npts], st[:npts]


def assert_trace(res, want, name):
    got = (res.iterations, res.trials, res.l_blocks, res.status)
    assert got == (want.iterations, want.trials, want.l_blocks, want.status), (name, got)
    assert np.array([res.chi2_first, res.chi2_last, res.lam]).tobytes() == np.array([want.chi2_first, want.chi2_last, want.lam], np.float64).tobytes(), name


def store_for(afv, ctx, pos, flags, **kind):
    pts = afv.MapPoints(ctx, len(pos), **(kind or {"desc_bytes": 32}))
    on = np.nonzero(flags & G.SET)[0].astype(np.int32)
    pts.set(on, pos=pos[on])
    pts.set_flags(on, bad=(flags[on] & G.BAD) != 0)
    return pts


def expected_positions(pos, flags):
    """what the store reads back: the positions, 0 for an id that was never set"""
    return np.where((flags & G.SET)[:, None] != 0, pos, np.float32(0.0)).astype(np.float32)


def store_image(pts):
    g = pts.get(np.arange(pts.capacity, dtype=np.int32))
    return b"".join(np.ascontiguousarray(g[k]).tobytes() for k in sorted(g))


@pytest.mark.parametrize("name", sorted(SC.SCENES))
def test_constructed_scene_is_bit_equal_to_the_restatement(afv, gpu_ctx, name):
    sc, pr, want, _ = SC.solved(name)
    pos, flags, ids, ref = SC.points_for(sc)
    pts = store_for(afv, gpu_ctx, pos, flags)
    code, res, S_out, Tiw, xyz, st = call(afv, gpu_ctx, sc, pts, ids, ref)
    assert code == 0, (name, gpu_ctx.last_error() if hasattr(gpu_ctx, "last_error") else code)
    assert_trace(res, want, name)
    assert S_out.tobytes() == H.records(want.S).tobytes(), name
    assert Tiw.tobytes() == want.Tiw.tobytes(), name
    pos_ref = pos.copy()
    wx, ws = G.correct_points(pos_ref, flags, ids, ref, sc["S_init"], want.Swc)
    assert np.array_equal(st, ws) and xyz.tobytes() == wx.tobytes(), name
    assert pts.get(np.arange(len(pos), dtype=np.int32))["pos"].tobytes() == expected_positions(pos_ref, flags).tobytes(), name
    pts.close()


@pytest.mark.parametrize("name", sorted(SIZED))
def test_sized_scene_is_bit_equal_to_the_host_program(afv, gpu_ctx, host_program, name):
    sc = SIZED[name]()
    want = H.run_host(host_program, sc)
    assert want.plan == 0
    pos, flags, ids, ref = SC.points_for(sc, n=50, cap=80)
    pts = store_for(afv, gpu_ctx, pos, flags)
    code, res, S_out, Tiw, xyz, st = call(afv, gpu_ctx, sc, pts, ids, ref)
    assert code == 0, name
    assert_trace(res, want, name)
    assert want.iterations >= 1 and want.status == G.OK
    assert S_out.tobytes() == want.S.tobytes() and Tiw.tobytes() == want.Tiw.tobytes(), name
    pos_host = pos.copy()
    wx, ws = H.host_correct(host_program, pos_host, flags, ids, ref, H.records(sc["S_init"]), want.Swc)
    assert np.array_equal(st, ws) and xyz.tobytes() == wx.tobytes(), name
    assert pts.get(np.arange(len(pos), dtype=np.int32))["pos"].tobytes() == expected_positions(pos_host, flags).tobytes(), name
    pts.close()


def test_sized_scenes_reach_the_edges_of_the_shape():
    cols = lambda name: [len(c) for c in SC.problem(SIZED[name]()).cols]
    assert max(cols("band_15")) == 16 and max(cols("band_16")) == 17 and max(cols("band_17")) == 18 and max(cols("band_0")) == 1 and max(cols("band_1")) == 2
    assert min(cols("chain_130_loop")[:-2]) == 2 and min(cols("chain_65_loop")[:-2]) == 2                                     # the loop edge fills every column
    pr = SC.problem(SIZED["hubs_63_64_65"]())
    assert sorted(len(pr.v_edges[i]) for i in range(3)) == [63, 64, 65]
    log = []
    sc = SIZED["floating_sized"]()
    G.optimize(SC.problem(sc), sc["iterations"], log=log)
    assert any(l.get("why") == "pivot" for l in log)


def test_fill_beyond_the_cap_is_refused_before_any_launch(afv, gpu_ctx):
    n = 600                                                                          # vertex 1 joined with every later one: 599 * 600 / 2 blocks
    I = (np.eye(3), np.zeros(3), 1.0)
    sc = SC.scene([I] * n, 0, [(k, 1) for k in range(2, n)], [I] * n)
    assert (n - 1) * n // 2 > afv._lib.ESS_MAX_L_BLOCKS
    pos, flags, ids, ref = SC.points_for(sc)
    pts = store_for(afv, gpu_ctx, pos, flags)
    before = store_image(pts)
    out = poisoned(n, len(ids))
    keep = [a.copy() for a in out]
    code, res, *_ = call(afv, gpu_ctx, sc, pts, ids, ref, out=out)
    assert code == -5                                                                # AFV_ECAPACITY
    assert all(a.tobytes() == b.tobytes() for a, b in zip(out, keep)) and bytes(res) == b"\xa5" * C.sizeof(res)
    assert store_image(pts) == before
    pts.close()


@pytest.mark.parametrize("npts", [0, 1, 63, 64, 65, 257])
@pytest.mark.parametrize("kind", ["binary", "float"])
def test_point_correction_through_both_entries(afv, gpu_ctx, npts, kind):
    sc, pr, want, _ = SC.solved("drifted_loop")
    kw = {"float_dim": 64} if kind == "float" else {"desc_bytes": 32}
    pos, flags, ids, ref = SC.points_for(sc, n=npts, cap=300, seed=npts)
    a, b, c = (store_for(afv, gpu_ctx, pos, flags, **kw) for _ in range(3))
    before = store_image(c)
    pos_ref = pos.copy()
    wx, ws = G.correct_points(pos_ref, flags, ids, ref, sc["S_init"], want.Swc)
    code, res, S_out, Tiw, xyz, st = call(afv, gpu_ctx, sc, a, ids, ref)                       # inside the essential-graph call
    assert code == 0 and np.array_equal(st, ws) and xyz.tobytes() == wx.tobytes()
    every = np.arange(len(pos), dtype=np.int32)
    assert a.get(every)["pos"].tobytes() == expected_positions(pos_ref, flags).tobytes()
    st2 = b.correct_sim3(ids, ref, H.records(sc["S_init"]), H.records(want.Swc))             # the call of its own
    assert np.array_equal(st2, ws) and b.get(every)["pos"].tobytes() == expected_positions(pos_ref, flags).tobytes()
    code, _, _, _, xyz0, st0 = call(afv, gpu_ctx, sc, c, ids, ref, write_points=0)            # write_points = 0 leaves the store
    assert code == 0 and xyz0.tobytes() == wx.tobytes() and np.array_equal(st0, ws) and store_image(c) == before
    if npts >= 6:
        assert set(ws) == {G.MOVED, G.BAD_OR_UNSET, G.NO_PAIR}
    for s in (a, b, c):
        s.close()


def test_two_calls_in_a_row_give_equal_answers(afv, gpu_ctx):
    sc = SC.SCENES["drifted_loop"]()
    one, two = call(afv, gpu_ctx, sc), call(afv, gpu_ctx, sc)
    assert one[0] == two[0] == 0 and bytes(one[1]) == bytes(two[1])
    assert one[2].tobytes() == two[2].tobytes() and one[3].tobytes() == two[3].tobytes()


def test_every_refusal_leaves_the_outputs_and_the_store_untouched(afv, gpu_ctx):
    L = afv._lib
    sc = SC.SCENES["double_edges"]()
    pos, flags, ids, ref = SC.points_for(sc)
    pts = store_for(afv, gpu_ctx, pos, flags)
    other = afv.Context(max_width=640, max_height=480, max_batch=1)
    foreign = afv.MapPoints(other, 64)
    before = store_image(pts)
    nk, ne = len(sc["S_init"][2]), len(sc["v0"])
    S, M = H.records(sc["S_init"]), H.records(sc["meas"])

    def changed(a, i, j, v):
        a = a.copy()
        a[i, j] = v
        return a

    def prm(**kw):
        p = L.sized(L.EssParams)
        p.iterations, p.lambda_init, p.fix_scale, p.write_points = 5, 1e-16, 0, 1
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    v0 = np.ascontiguousarray(sc["v0"], np.int32)
    twice = ids.copy()
    twice[2] = twice[0]
    cases = dict(
        null_S=dict(S=None), null_prm=dict(prm=None), null_res=dict(res=None), null_S_out=dict(S_out=None), null_Tiw=dict(Tiw=None),
        null_v0=dict(v0=None), null_meas=dict(M=None), null_ids=dict(ids_raw=None), null_ref=dict(ref_raw=None), null_xyz=dict(xyz=None), null_status=dict(st=None),
            np_beyond_capacity=dict(npts=65), null_store=dict(points_raw=None),
        struct_size=dict(prm=prm(struct_size=12)), nk_zero=dict(nk=0), nk_cap=dict(nk=L.ESS_MAX_KF + 1), ne_cap=dict(ne=L.ESS_MAX_EDGES + 1),
        ne_negative=dict(ne=-1), np_negative=dict(npts=-1), iterations=dict(prm=prm(iterations=-1)), fix_scale=dict(prm=prm(fix_scale=2)),
        write_points=dict(prm=prm(write_points=3)), lambda_zero=dict(prm=prm(lambda_init=0.0)), lambda_nan=dict(prm=prm(lambda_init=float("nan"))),
        fixed_low=dict(fixed=-1), fixed_high=dict(fixed=nk), edge_end=dict(v0=changed(v0[:, None], 1, 0, nk).reshape(-1)),
        edge_negative=dict(v0=changed(v0[:, None], 1, 0, -1).reshape(-1)), self_edge=dict(v0=np.ascontiguousarray(sc["v1"], np.int32)),
        meas_nan=dict(M=changed(M, 2, 4, np.nan)), meas_scale=dict(M=changed(M, 1, 12, 0.0)), init_inf=dict(S=changed(S, 1, 9, np.inf)),
        init_scale=dict(S=changed(S, 3, 12, -1.0)), foreign_store=dict(points_raw=foreign.handle), id_range=dict(ids_raw=changed(ids[:, None], 0, 0, 64).reshape(-1)),
        id_twice=dict(ids_raw=twice), ref_range=dict(ref_raw=changed(ref[:, None], 0, 0, nk).reshape(-1)), ref_low=dict(ref_raw=changed(ref[:, None], 0, 0, -2).reshape(-1)),
    )
    for name, over in cases.items():
        out = poisoned(nk, len(ids))
        keep = [a.copy() for a in out]
        code, res, *_ = call(afv, gpu_ctx, sc, pts, ids, ref, out=out, **over)
        assert code == -1, (name, code)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(out, keep)), name
        if over.get("res", 1) is not None:
            assert bytes(res) == b"\xa5" * C.sizeof(res), name
        assert store_image(pts) == before, name
    # the point correction of its own
    A = H.records(sc["S_init"])
    for name, args in dict(id_range=(changed(ids[:, None], 0, 0, -1).reshape(-1), ref, A, A), id_twice=(twice, ref, A, A),
                           pair_range=(ids, changed(ref[:, None], 0, 0, nk).reshape(-1), A, A), sim3_nan=(ids, ref, changed(A, 0, 0, np.nan), A),
                           sim3_scale=(ids, ref, A, changed(A, 1, 12, 0.0))).items():
        with pytest.raises(L.AfvError) as err:
            pts.correct_sim3(*args)
        assert err.value.code == -1, name
        assert store_image(pts) == before, name
    for s in (pts, foreign):
        s.close()
    other.close()


def test_python_layer_builds_the_list_and_optimises(afv, gpu_ctx):
    """OptimizeEssentialGraph over keyframe dicts: the list of essential_graph_edges, optimised, equals the restatement on the same list"""
    n = 10
    truth = SC.circle(n, 1.1)
    key_ids = [3 * k for k in range(n)]
    kfs = [dict(id=key_ids[k], Rcw=(SC.rot([0.01 * k, 0, 0]) @ truth[k][0]).astype(np.float32), tcw=(truth[k][1] / truth[k][2]).astype(np.float32))
           for k in range(n)]
    non_corrected = {key_ids[n - 1]: (kfs[n - 1]["Rcw"].astype(np.float64), kfs[n - 1]["tcw"].astype(np.float64), np.float64(1.0))}
    corrected = {key_ids[n - 1]: truth[n - 1]}
    graph = dict(parent={key_ids[k]: (key_ids[k - 1] if k else None) for k in range(n)}, loop_edges={},
                 covisibles={key_ids[k]: [key_ids[j] for j in (k - 2, k - 1, k + 1) if 0 <= j < n] + ([key_ids[1]] if k == n - 1 else []) for k in range(n)})
    loop_connections = {key_ids[n - 1]: [(key_ids[0], 30), (key_ids[1], 120)]}
    pos, flags, ids, _ = SC.points_for(dict(S_init=SC.pack(truth)), n=30)
    ref_ids = np.array([key_ids[i % n] if i % 5 else -1 for i in range(len(ids))])
    pts = store_for(afv, gpu_ctx, pos, flags)
    out = afv.OptimizeEssentialGraph(gpu_ctx, pts, kfs, key_ids[0], key_ids[n - 1], non_corrected, corrected, loop_connections, graph, False, ids, ref_ids)
    edges = out["edges"]
    assert (key_ids[n - 1], key_ids[0]) in [(e[0], e[1]) for e in edges[:2]] and len(edges) == 2 + (n - 1) + (n - 2)
    at = {k: i for i, k in enumerate(key_ids)}
    S_init = [corrected[i] if i in corrected else (k["Rcw"].astype(np.float64), k["tcw"].astype(np.float64), 1.0) for i, k in zip(key_ids, kfs)]
    sc = SC.scene(S_init, 0, [(at[e[0]], at[e[1]]) for e in edges], None, meas=[e[2] for e in edges])
    want = G.essential_graph(SC.problem(sc))
    assert out["CorrectedSiw"].tobytes() == H.records(want.S).tobytes() and out["Tiw"].tobytes() == want.Tiw_f.tobytes()
    assert out["result"].iterations == want.iterations and out["result"].trials == want.trials
    pos_ref = pos.copy()
    ref = np.array([at.get(int(r), -1) for r in ref_ids], np.int32)
    wx, ws = G.correct_points(pos_ref, flags, ids, ref, sc["S_init"], want.Swc)
    assert np.array_equal(out["point_status"], ws) and out["xyz"].tobytes() == wx.tobytes()
    pts.close()
