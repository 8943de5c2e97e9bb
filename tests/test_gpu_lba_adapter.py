"""-m gpu: afv::LocalBundleAdjustment / afv::BundleAdjustment of adapter/afv_adapter.hpp as a plain C++ process (adapter/lba_selftest): a
constructed scene goes in as a file; the trace, the pose and point doubles, the per-observation states, vToErase and the store's
positions come out and equal what the Python classes (afv.LocalBundleAdjustment / afv.BundleAdjustment) answer on the same scene, bit
for bit - and both equal the restatement (tests/_lba_ref.py)."""
import os
import subprocess

import numpy as np
import pytest

import _lba_scenes as S
from test_gpu_lba import Rig

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "anyfeature-vslam_amd", "adapter", "lba_selftest")


def _hx(v):
    return float(np.float32(v)).hex()


def world_file(sc, slots, path):
    cap = max(len(f["x"]) for f in sc.feats) + 2
    lines = ["%d %d %d %d %d %d %d %d" % (cap, sc.nk, sc.np, sc.store_cap, sc.ne, int(sc.checks), sc.iterations[0], int(sc.robust[0]))]
    for k in range(sc.nk):
        f = sc.feats[k]
        lines.append("%d %d %d" % (slots[k], int(k >= sc.nf), len(f["x"])))
        lines.append(" ".join(_hx(v) for v in sc.cams[k]))
        lines += ["%s %s %s %s" % (_hx(f["x"][i]), _hx(f["y"][i]), _hx(f["ur"][i]), _hx(f["inf"][i])) for i in range(len(f["x"]))]
    lines += ["%d %s %s %s %d" % (sc.ids[p], _hx(sc.pos[p, 0]), _hx(sc.pos[p, 1]), _hx(sc.pos[p, 2]), int(not sc.p_ok[p])) for p in range(sc.np)]
    lines += ["%d %d %d" % (sc.ids[sc.e_pt[e]], slots[sc.e_kf[e]], sc.e_idx[e]) for e in range(sc.ne)]
    path.write_text("\n".join(lines) + "\n")


@pytest.mark.parametrize("name", ["local", "start_up"])
def test_cpp_adapter_answers_as_the_python_class(afv, gpu_ctx, tmp_path, name):
    assert os.path.exists(BIN), "lba_selftest is not built: __graft_entry__.build() compiles it"
    if name == "local":
        sc = S.make(seed=51, stereo_kfs=(1, 4), outliers=[(3, 0, -30.0), (11, 4, 25.0)], dropped=(6,))
    else:
        sc = S.make(nk=2, nf=1, npts=50, seed=52, iterations=(20, 0), robust=(False, False), checks=False, shake=0.05)
    rig = Rig(afv, gpu_ctx, sc)
    try:
        # a dropped point arrives in the selftest as a BAD point, here as one that was never set: both are dropped by the same rule
        slots = [int(s) for s in rig.slots]
        inp = tmp_path / "world.txt"
        world_file(sc, slots, inp)
        r = subprocess.run([BIN, str(inp)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        cams = {slots[k]: dict(Rcw=sc.cams[k, :9], tcw=sc.cams[k, 9:12], fx=sc.cams[k, 12], fy=sc.cams[k, 13], cx=sc.cams[k, 14], cy=sc.cams[k, 15],
                               mbf=sc.cams[k, 16]) for k in range(sc.nk)}
        obs = [(int(sc.ids[sc.e_pt[e]]), slots[sc.e_kf[e]], int(sc.e_idx[e])) for e in range(sc.ne)]
        if sc.checks:
            poses, xyz, erase, trace = afv.LocalBundleAdjustment(rig.table, rig.points, slots[:sc.nf], slots[sc.nf:], cams, sc.ids, obs)
        else:
            poses, xyz, trace = afv.BundleAdjustment(rig.table, rig.points, [(s, k >= sc.nf) for k, s in enumerate(slots)], cams, sc.ids, obs,
                                                     nIterations=sc.iterations[0], robust=bool(sc.robust[0]))
            erase = []
        stored = rig.points.get(sc.ids)["pos"]
    finally:
        rig.close()
    want = ["T %d %d %d %d %d %d %d %d" % (*trace["iterations"], *trace["trials"], trace["n_edges"], trace["n_removed_first"], trace["n_erase"],
                                          trace["stopped"]),
            "D " + " ".join(float(v).hex() for v in trace["chi2"] + trace["lam"])]
    want += ["K %d " % s + " ".join(float(v).hex() for v in list(poses[s][0].reshape(9)) + list(poses[s][1])) for s in slots[:sc.nf]]
    want += ["X " + " ".join(float(v).hex() for v in xyz[p]) for p in range(sc.np)]
    want.append("S " + " ".join(str(int(v)) for v in trace["edge_state"]))
    want.append(("E " + " ".join("%d:%d" % e for e in erase)).rstrip())
    ok = sc.p_ok.astype(bool)
    # the bad point of the selftest keeps the position it was given; the unset one here reads 0
    want += ["P " + " ".join(float(v).hex() for v in (stored[p] if ok[p] else sc.pos[p])) for p in range(sc.np)]
    got = [l.rstrip() for l in r.stdout.splitlines()]
    parse = lambda ls: [float.fromhex(v) if "x" in v or "nan" in v or "inf" in v else v for l in ls for v in l.split()]
    assert parse(got) == parse(want)
    assert len(got) == len(want)
    ref = sc.solve()
    assert xyz.tobytes() == ref.xyz.tobytes() and np.array_equal(trace["edge_state"], ref.state)
    if name == "local":
        assert ref.n_erase >= 2 and len(erase) == ref.n_erase and ref.n_edges == sc.ne - 6
