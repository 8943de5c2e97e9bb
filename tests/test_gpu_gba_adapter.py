"""-m gpu: afv::GlobalBundleAdjustment / afv::CorrectPointsSE3 of adapter/afv_adapter.hpp as a plain C++ process (adapter/gba_selftest): a
constructed map with more than 64 free keyframes goes in as a file; the trace, the pose and point doubles, the per-observation states,
the store's positions after the adjustment, the correction's statuses and the store's positions after it come out and equal what the
Python route (afv.GlobalBundleAdjustment, MapPoints.correct_se3) answers on the same map, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import _gba_scenes as GS
from test_gpu_gba import seeded_transforms
from test_gpu_lba import Rig

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "anyfeature-vslam_amd", "adapter", "gba_selftest")


def _hx(v):
    return float(np.float32(v)).hex()


def world_file(sc, slots, write_points, T, cids, pair, path):
    cap = max(len(f["x"]) for f in sc.feats) + 2
    lines = ["%d %d %d %d %d %d %d %d %d %d" % (cap, sc.nk, sc.np, sc.store_cap, sc.ne, sc.iterations[0], int(sc.robust[0]), int(write_points), T.shape[1],
                                                len(cids))]
    for k in range(sc.nk):
        f = sc.feats[k]
        lines.append("%d %d %d" % (slots[k], int(k >= sc.nf), len(f["x"])))
        lines.append(" ".join(_hx(v) for v in sc.cams[k]))
        lines += ["%s %s %s %s" % (_hx(f["x"][i]), _hx(f["y"][i]), _hx(f["ur"][i]), _hx(f["inf"][i])) for i in range(len(f["x"]))]
    lines += ["%d %s %s %s %d" % (sc.ids[p], _hx(sc.pos[p, 0]), _hx(sc.pos[p, 1]), _hx(sc.pos[p, 2]), int(not sc.p_ok[p])) for p in range(sc.np)]
    lines += ["%d %d %d" % (sc.ids[sc.e_pt[e]], slots[sc.e_kf[e]], sc.e_idx[e]) for e in range(sc.ne)]
    lines += [" ".join(_hx(v) for v in list(T[0, q]) + list(T[1, q])) for q in range(T.shape[1])]
    lines += ["%d %d" % (i, q) for i, q in zip(cids, pair)]
    path.write_text("\n".join(lines) + "\n")


@pytest.mark.parametrize("write_points", [0, 1])
def test_cpp_adapter_answers_as_the_python_route(afv, gpu_ctx, tmp_path, write_points):
    assert os.path.exists(BIN), "gba_selftest is not built: __graft_entry__.build() compiles it"
    sc = GS.band(n_free=66, n_fixed=1, width=3, npts=66 * 4, seed=61, loop=2, dropped=(6,), **GS.LOOP)
    T = seeded_transforms(3, 9)
    cids = [int(i) for i in sc.ids[:12]]
    pair = [q % 3 for q in range(12)]
    pair[4] = -1
    rig = Rig(afv, gpu_ctx, sc)
    try:
        slots = [int(s) for s in rig.slots]
        inp = tmp_path / "world.txt"
        world_file(sc, slots, write_points, T, cids, pair, inp)
        r = subprocess.run([BIN, str(inp)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        cams = {slots[k]: dict(Rcw=sc.cams[k, :9], tcw=sc.cams[k, 9:12], fx=sc.cams[k, 12], fy=sc.cams[k, 13], cx=sc.cams[k, 14], cy=sc.cams[k, 15],
                               mbf=sc.cams[k, 16]) for k in range(sc.nk)}
        obs = [(int(sc.ids[sc.e_pt[e]]), slots[sc.e_kf[e]], int(sc.e_idx[e])) for e in range(sc.ne)]
        poses, xyz, trace = afv.GlobalBundleAdjustment(rig.table, rig.points, [(s, k >= sc.nf) for k, s in enumerate(slots)], cams, sc.ids, obs,
                                                       nIterations=sc.iterations[0], robust=bool(sc.robust[0]), write_points=bool(write_points))
        stored = rig.points.get(sc.ids)["pos"].copy()
        st = rig.points.correct_se3(cids, pair, T[0], T[1])
        moved = rig.points.get(sc.ids)["pos"].copy()
    finally:
        rig.close()
    assert trace["iterations"][0] >= 1 and len(poses) == 66
    want = ["T %d %d %d %d %d %d %d %d" % (*trace["iterations"], *trace["trials"], trace["n_edges"], trace["n_removed_first"], trace["n_erase"],
                                          trace["stopped"]),
            "D " + " ".join(float(v).hex() for v in trace["chi2"] + trace["lam"])]
    want += ["K %d " % s + " ".join(float(v).hex() for v in list(poses[s][0].reshape(9)) + list(poses[s][1])) for s in slots[:sc.nf]]
    want += ["X " + " ".join(float(v).hex() for v in xyz[p]) for p in range(sc.np)]
    want.append("S " + " ".join(str(int(v)) for v in trace["edge_state"]))
    ok = sc.p_ok.astype(bool)
    # the bad point of the selftest keeps the position it was given; the unset one here reads 0
    want += ["P " + " ".join(float(v).hex() for v in (stored[p] if ok[p] else sc.pos[p])) for p in range(sc.np)]
    want.append("C " + " ".join(str(int(v)) for v in st))
    want += ["Q " + " ".join(float(v).hex() for v in (moved[p] if ok[p] else sc.pos[p])) for p in range(sc.np)]
    got = [l.rstrip() for l in r.stdout.splitlines()]
    parse = lambda ls: [float.fromhex(v) if "x" in v or "nan" in v or "inf" in v else v for l in ls for v in l.split()]
    assert parse(got) == parse(want)
    assert len(got) == len(want)
    L = afv._lib
    assert list(st[:8]) == [L.POINT_MOVED] * 4 + [L.POINT_NO_PAIR, L.POINT_MOVED, L.POINT_BAD_OR_UNSET, L.POINT_MOVED]
    assert (stored[ok].tobytes() == xyz[ok].astype(np.float32).tobytes()) == bool(write_points)
    assert moved[0].tobytes() != stored[0].tobytes()
