"""Mirror of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:771-1031, as LoopClosing::CorrectLoop calls it) over plain arrays and
the map-point store: afv_essential_graph (csrc/k_essgraph.hip), and of the point correction of CorrectLoop (LoopClosing.cc:487-516):
afv_points_correct_sim3 (MapPoints.correct_sim3).  Normative semantics, the quirk G-Q1 and the deviations G1-G11:
tests/_essgraph_ref.py and include/afv_hip.h ("Essential graph").

A Sim3 is (R [3, 3], t [3], s) in double, or a row of 13 doubles (R row-major, t, s); map(P) = s (R P) + t.
What stays with the host's map: SetPose from the returned poses, and UpdateNormalAndDepth of the moved points, which is
refresh.UpdateNormalAndDepth on the device.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ptr

F64 = np.float64


def sim3_records(S):
    """[(R, t, s)] or an [n, 13] array -> [n, 13] float64, the layout of afv_sim3d"""
    if isinstance(S, np.ndarray) and S.ndim == 2 and S.shape[1] == 13:
        return np.ascontiguousarray(S, F64)
    out = np.zeros((len(S), 13), F64)
    for i, (R, t, s) in enumerate(S):
        out[i, :9], out[i, 9:12], out[i, 12] = np.asarray(R, F64).reshape(9), np.asarray(t, F64).reshape(3), F64(s)
    return out


def sim3_inverse(S):
    """Sim3::inverse: (R^T, R^T (t * (-1 / s)), 1 / s), in the operator order of the restatement"""
    R, t, s = np.asarray(S[0], F64).reshape(3, 3), np.asarray(S[1], F64).reshape(3), F64(S[2])
    m = F64(-1.0) / s
    tm = [t[0] * m, t[1] * m, t[2] * m]
    ti = np.array([R[0, i] * tm[0] + (R[1, i] * tm[1] + R[2, i] * tm[2]) for i in range(3)], F64)
    return np.ascontiguousarray(R.T), ti, F64(1.0) / s


def sim3_mul(A, B):
    """Sim3::operator*: A * B"""
    Ra, ta, sa = np.asarray(A[0], F64).reshape(3, 3), np.asarray(A[1], F64).reshape(3), F64(A[2])
    Rb, tb, sb = np.asarray(B[0], F64).reshape(3, 3), np.asarray(B[1], F64).reshape(3), F64(B[2])
    R = np.array([[Ra[i, 0] * Rb[0, j] + (Ra[i, 1] * Rb[1, j] + Ra[i, 2] * Rb[2, j]) for j in range(3)] for i in range(3)], F64)
    t = np.array([sa * (Ra[i, 0] * tb[0] + (Ra[i, 1] * tb[1] + Ra[i, 2] * tb[2])) + ta[i] for i in range(3)], F64)
    return R, t, sa * sb


def essential_graph_edges(key_ids, parent, loop_edges, covisibles, loop_connections, Scw, non_corrected, loop_id, cur_id, min_feat=100):
    """The edge list of :835-971 over plain inputs, in the reference's order.
    key_ids: the keyIds of the keyframes that are not bad, ascending (vpKFs); parent {id: id | None}; loop_edges {id: ids};
    covisibles {id: [ids]} = GetCovisiblesByWeight(minFeat) in its order; loop_connections {id: [(id_j, weight of the pair)]}, walked in
    ascending id as the reference's maps are; Scw {id: Sim3} = vScw (CorrectedSim3 or (Rcw, tcw, 1)); non_corrected {id: Sim3}.
    Returns [(id_i, id_j, Sji)], id_i the vertex of setVertex(0, ...):
      the loop connections first, unless (id_i != cur_id or id_j != loop_id) and weight < min_feat; each fills sInsertedEdges;
      then per keyframe its spanning-tree edge to the parent, its loop edges to lower ids in ascending id (G11: the reference's set is
      ordered by pointer), and its covisibility edges to lower ids that are
      not its parent, not its child, not a loop edge, not bad (not in key_ids) and not in sInsertedEdges.
    Sji = Sjw * Swi, with the non-corrected pose of either end where one exists (the loop connections: vScw of both)."""
    ids = set(key_ids)
    out, inserted = [], set()
    rel = lambda Sjw, Siw: sim3_mul(Sjw, sim3_inverse(Siw))
    for i in sorted(loop_connections):
        for j, w in sorted(loop_connections[i], key=lambda c: c[0]):
            if (i != cur_id or j != loop_id) and w < min_feat:
                continue
            out.append((i, j, rel(Scw[j], Scw[i])))
            inserted.add((min(i, j), max(i, j)))
    pick = lambda j: non_corrected[j] if j in non_corrected else Scw[j]
    for i in key_ids:
        Siw = pick(i)
        p = parent.get(i)
        if p is not None:
            out.append((i, p, rel(pick(p), Siw)))
        le = loop_edges.get(i, ())
        for j in sorted(le):
            if j < i:
                out.append((i, j, rel(pick(j), Siw)))
        for n in covisibles.get(i, ()):
            if n == p or parent.get(n) == i or n in le or n not in ids or not n < i:
                continue
            if (min(i, n), max(i, n)) in inserted:
                continue
            out.append((i, n, rel(pick(n), Siw)))
    return out


def essential_graph(ctx, points, S_init, fixed, edge_v0, edge_v1, edge_meas, iterations=20, lambda_init=1e-16, fix_scale=False, point_ids=None,
                    point_ref=None, write_points=True):
    """afv_essential_graph as it is.  Returns (result: EssResult, S_out [nk, 13], Tiw [nk, 12] float64, xyz [np, 3] float64, point_status [np])"""
    lib = ctx.lib
    S = sim3_records(S_init)
    M = sim3_records(edge_meas)
    v0, v1 = np.ascontiguousarray(edge_v0, np.int32).reshape(-1), np.ascontiguousarray(edge_v1, np.int32).reshape(-1)
    nk, ne = len(S), len(v0)
    if len(v1) != ne or len(M) != ne:
        raise ValueError("essential_graph: one v1 and one measurement per edge are expected")
    ids = np.zeros(0, np.int32) if point_ids is None else np.ascontiguousarray(point_ids, np.int32).reshape(-1)
    ref = np.zeros(0, np.int32) if point_ref is None else np.ascontiguousarray(point_ref, np.int32).reshape(-1)
    npts = len(ids)
    if len(ref) != npts:
        raise ValueError("essential_graph: one reference per point is expected")
    if npts and points is None:
        raise ValueError("essential_graph: points to correct need their store")
    pad = lambda a: a if len(a) else np.zeros((4,) + a.shape[1:], a.dtype)
    prm = _lib.EssParams(C.sizeof(_lib.EssParams), int(iterations), float(lambda_init), int(bool(fix_scale)), int(bool(write_points)))
    res = _lib.EssResult()
    S_out, Tiw = np.zeros((nk, 13), F64), np.zeros((nk, 12), F64)
    xyz, st = np.zeros((max(npts, 1), 3), F64), np.zeros(max(npts, 1), np.uint8)
    ctx.check(lib.afv_essential_graph(ctx.handle, None if points is None else points.handle, ptr(S), nk, int(fixed), ptr(pad(v0)), ptr(pad(v1)),
                                      ptr(pad(M)), ne, C.byref(prm), ptr(pad(ids)), ptr(pad(ref)), npts, C.byref(res), ptr(S_out), ptr(Tiw), ptr(xyz),
                                      ptr(st)), "afv_essential_graph")
    return res, S_out, Tiw, xyz[:npts], st[:npts]


def OptimizeEssentialGraph(ctx, points, keyframes, loop_kf, cur_kf, NonCorrectedSim3, CorrectedSim3, loop_connections, graph, fix_scale,
                           point_ids=None, point_ref=None, iterations=20, lambda_init=1e-16, min_feat=100, write_points=True):
    """Optimizer::OptimizeEssentialGraph.  keyframes: [{id, Rcw [3, 3], tcw [3]}] of the keyframes that are not bad, ascending keyId; loop_kf /
    cur_kf: keyIds; NonCorrectedSim3 / CorrectedSim3: {keyId: Sim3}; loop_connections: {keyId: [(keyId, weight)]}; graph: {parent: {id: id |
    None}, loop_edges: {id: ids}, covisibles: {id: [ids]}}; point_ref: per point the keyId of mnCorrectedReference (when mnCorrectedByKF is
    the current keyframe) or of mpRefKF, -1 for none.  Returns a dict: Tiw [nk, 12] float32 (what SetPose takes), Tiw_double, CorrectedSiw [nk,
    13], xyz [np, 3], point_status [np], edges (the list that was optimised), result (EssResult: the trace)."""
    key_ids = [int(k["id"]) for k in keyframes]
    if any(b <= a for a, b in zip(key_ids, key_ids[1:])):
        raise ValueError("OptimizeEssentialGraph: the keyframes come in ascending keyId")
    pos_of = {k: i for i, k in enumerate(key_ids)}
    Scw = {}
    for k in keyframes:
        i = int(k["id"])
        Scw[i] = CorrectedSim3[i] if i in CorrectedSim3 else (np.asarray(k["Rcw"], np.float32).astype(F64).reshape(3, 3),
                                                             np.asarray(k["tcw"], np.float32).astype(F64).reshape(3), F64(1.0))
    edges = essential_graph_edges(key_ids, graph.get("parent", {}), graph.get("loop_edges", {}), graph.get("covisibles", {}), loop_connections, Scw,
                                  NonCorrectedSim3, int(loop_kf), int(cur_kf), min_feat)
    ref = None
    if point_ids is not None:
        ref = np.array([pos_of.get(int(r), -1) for r in np.asarray(point_ref).reshape(-1)], np.int32)
    res, S_out, Tiw, xyz, st = essential_graph(ctx, points, [Scw[i] for i in key_ids], pos_of[int(loop_kf)], [pos_of[e[0]] for e in edges],
                                               [pos_of[e[1]] for e in edges], [e[2] for e in edges], iterations, lambda_init, fix_scale, point_ids, ref,
                                               write_points)
    return dict(Tiw=Tiw.astype(np.float32), Tiw_double=Tiw, CorrectedSiw=S_out, xyz=xyz, point_status=st, edges=edges, result=res)
